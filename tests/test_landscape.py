"""Folding landscape, CPU side: the fixture (tools/make_golden_landscape.py: scikit-learn's and scipy's recorded results on the
reference's two example graphs), the numpy statement of the iteration the kernels implement, the readers and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _landscape_np as NP
from conftest import GOLD, ROOT

EXAMPLES = ["example_rafft.out", "example_rafft_20.out"]


@pytest.fixture(scope="module")
def fx():
    return NP.fixture()


@pytest.mark.parametrize("name", EXAMPLES)
def test_fixture_distances_are_the_pair_set_definition(fx, name):
    from rafft_amd import landscape as LS, utils
    ex = fx["examples"][name]
    fp, _ = utils.parse_rafft_output(os.path.join(GOLD, name))
    structs, energies = LS.unique_structures(fp)
    assert structs == ex["structs"] and np.array_equal(energies, np.array(ex["energies"]))
    D = np.array(ex["D"])
    want = np.array([[NP.bp_distance(a, b) for b in structs] for a in structs])
    assert np.array_equal(D, want)
    assert np.array_equal(D, D.T) and not D.diagonal().any() and (D[~np.eye(len(D), dtype=bool)] >= 1).all()
    t, npairs = NP.pair_tables(structs)
    assert np.array_equal(NP.distance_rows(t, npairs, range(len(structs))), D)


def test_numpy_smacof_reproduces_every_fixture_case(fx):
    n_cases = 0
    for name in EXAMPLES:
        ex = fx["examples"][name]
        D = np.array(ex["D"])
        for c in ex["cases"]:
            X, stress, n_iter, _, crit = NP.smacof(D, np.array(c["x0"]), c["max_iter"], c["eps"])
            assert n_iter == c["n_iter"], (name, c["seed"], c["max_iter"])
            assert np.abs(X - np.array(c["x"])).max() <= 10 * fx["delta_x"]
            assert abs(stress - c["stress"]) <= 10 * max(fx["delta_stress"], 1e-15) * c["stress"]
            assert all(abs(v - c["eps"]) >= 1e-6 * c["eps"] for v in c["criterion_last2"])
            n_cases += 1
    assert n_cases == 12


def test_torch_restatement_is_the_numpy_one(fx):
    """test_gpu_landscape.py runs the big graphs through smacof_torch (float64 on CPU threads): the same iteration"""
    ex = fx["examples"]["example_rafft_20.out"]
    c = [c for c in ex["cases"] if c["max_iter"] == 5000][0]
    X, stress, n_iter, _, _ = NP.smacof_torch(np.array(ex["D"]), np.array(c["x0"]), c["max_iter"], c["eps"])
    assert n_iter == c["n_iter"] and np.abs(X - np.array(c["x"])).max() <= 10 * fx["delta_x"]


@pytest.mark.parametrize("name", EXAMPLES)
def test_documented_start_rule_gives_the_reference_positions(fx, name):
    from rafft_amd import landscape as LS
    ex = fx["examples"][name]
    p = ex["pipeline"]
    D = np.array(ex["D"])
    runs = [NP.smacof(D, x0, 5000, 1e-9)[:3] for x0 in LS.draw_starts(len(D), p["n_init"], 3)]
    assert [r[2] for r in runs] == [s["n_iter"] for s in p["starts"]]
    np.testing.assert_allclose([r[1] for r in runs], [s["stress"] for s in p["starts"]], rtol=1e-12)
    best = int(np.argmin([r[1] for r in runs]))
    assert best == p["winner"] and runs[best][2] == p["n_iter"]
    assert np.abs(runs[best][0] - np.array(p["pos"])).max() <= 10 * fx["delta_x"]
    if name == "example_rafft_20.out":
        assert abs(p["stress"] - 24698.8305) < 1e-3 and p["n_iter"] == 149 and p["winner"] == 3


def test_readers(tmp_path):
    from rafft_amd import landscape as LS, utils
    bar = tmp_path / "bar.out"
    bar.write_text("     GGGAAACCC\n   1 (((...)))  -1.20    0  10.00\n   2 .........   0.00    1   1.20\n")
    fp, seq = LS.parse_barrier_output(str(bar))
    assert seq == "GGGAAACCC" and [(s.str_struct, s.energy) for s in fp[0]] == [("(((...)))", -1.2), (".........", 0.0)]
    sub = tmp_path / "sub.out"
    sub.write_text("GGGAAACCC -120 100\n" + "".join(f"{'(' * k}{'.' * (9 - 2 * k)}{')' * k} {-k / 10:.2f}\n" for k in range(4)) * 25)
    full, _ = LS.parse_subopt_output(str(sub))
    assert len(full[0]) == 100 and full[0][1].str_struct == "(.......)" and full[0][1].energy == -0.1
    a, _ = LS.parse_subopt_output(str(sub), 0.3, seed=11)
    b, _ = LS.parse_subopt_output(str(sub), 0.3, seed=11)
    c, _ = LS.parse_subopt_output(str(sub), 0.3, seed=12)
    assert [s.str_struct for s in a[0]] == [s.str_struct for s in b[0]] and 10 < len(a[0]) < 55
    assert [s.str_struct for s in a[0]] != [s.str_struct for s in c[0]] or len(a[0]) != len(c[0])
    # the binary side-car carries the same graph as the text
    fp, seq = utils.parse_rafft_output(os.path.join(GOLD, "example_rafft.out"))
    utils.write_sidecar(str(tmp_path / "g.bin"), seq, fp)
    fp2, _ = utils.read_sidecar(str(tmp_path / "g.bin"), text_energies=True)
    assert LS.unique_structures(fp2)[0] == LS.unique_structures(fp)[0]


def test_cli_table_and_outputs(fx, tmp_path, capsys):
    from rafft_amd import landscape as LS
    src = os.path.join(GOLD, "example_rafft.out")
    ex = fx["examples"]["example_rafft.out"]
    assert LS.main([src, "--grid", "16"], compute=NP.tps_numpy_compute) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == len(ex["structs"]) + 1 and lines[-1].startswith("# stress ")
    p = ex["pipeline"]
    for line, s, e, xy in zip(lines, ex["structs"], ex["energies"], p["pos"]):
        f = line.split()
        assert len(f) == 4 and f[0] == s and f[1] == f"{e:.1f}" and f[2] == f"{xy[0]:.6f}" and f[3] == f"{xy[1]:.6f}"
    assert lines[-1].split() == ["#", "stress", f"{p['stress']:.2f}", "iterations", str(p["n_iter"]), "start", str(p["winner"]),
                                 "structures", str(len(ex["structs"]))]
    table, grid = tmp_path / "t.tsv", tmp_path / "z.npy"
    assert LS.main([src, "--grid", "16", "--table", str(table), "--grid-out", str(grid), "--seed", "4", "--n_init", "2", "--max_iter", "30",
                    "--eps", "0"], compute=NP.tps_numpy_compute) == 0
    assert capsys.readouterr().out == ""
    assert table.read_text().splitlines()[-1].split()[4] == "30"
    assert np.load(grid).shape == (17, 16)


def test_cli_bar_selects_the_barrier_reader(tmp_path, capsys):
    from rafft_amd import landscape as LS
    bar = tmp_path / "bar.out"
    bar.write_text("     GGGAAACCCAAA\n   1 (((...)))...  -1.20    0  10.00\n   2 ............   0.00    1   1.20\n"
                   "   3 .((...))....  -0.40    1   1.20\n   4 ..(......)..   0.90    1   1.20\n")
    assert LS.main([str(bar), "--bar", "--grid", "8", "--max_iter", "20"], compute=NP.tps_numpy_compute) == 0
    lines = capsys.readouterr().out.splitlines()
    assert [l.split()[0] for l in lines[:-1]] == ["(((...)))...", "............", ".((...))....", "..(......).."]


def test_cli_out_writes_a_picture_or_says_why(tmp_path, capsys):
    from rafft_amd import landscape as LS
    png = tmp_path / "l.png"
    rc = LS.main([os.path.join(GOLD, "example_rafft.out"), "--grid", "24", "-o", str(png)], compute=NP.tps_numpy_compute)
    cap = capsys.readouterr()
    assert rc == 0 and len(cap.out.splitlines()) == 15
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        assert "matplotlib" in cap.err and not png.exists()
    else:
        assert png.stat().st_size > 1000 and png.read_bytes()[:4] == b"\x89PNG"


def test_module_imports_neither_sklearn_nor_oracle():
    code = ("import sys; import rafft_amd.landscape as L; import rafft_amd; "
            "bad = [m for m in sys.modules if m.split('.')[0] in ('sklearn', 'oracle', 'scipy', 'matplotlib')]; "
            "assert not bad, bad; assert callable(rafft_amd.folding_landscape) and rafft_amd.landscape is L")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_native_exports_and_source_list():
    from rafft_amd import _native, build
    for name in ("rafft_landscape_distances", "rafft_landscape_mds", "rafft_landscape_surface", "rafft_landscape_counters"):
        assert name in _native.EXPORTS
    assert "rafft_landscape.hip" in build.SOURCES
    assert os.access(os.path.join(ROOT, "bin", "rafft_landscape"), os.X_OK)
