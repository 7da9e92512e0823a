"""The host side of the batch kinetics (rafft_kin_batch, rafft_kin.kinetics_batch, `rafft --kin`): the one schedule helper, the
record's layout, the option surface.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from rafft_amd import _native, cli, rafft_kin
from conftest import ROOT


def literal_schedule(sample_times, substeps):
    """the m / h lines of solve_master_equation as they stood before the helper existed"""
    t_now, ms, hs = 0.0, [], []
    for t in sample_times:
        m = max(1, int(np.ceil(substeps * (np.log(float(t) / t_now) / 0.3 if t_now > 0 else 1.0))))
        h = (float(t) - t_now) / m
        t_now = float(t)
        ms.append(m)
        hs.append(h)
    return ms, hs


IRREGULAR = [1e-3, 1.5e-3, 0.2, 0.2000001, 7.0, 1e4, 3e11]


@pytest.mark.parametrize("substeps", [1, 4, 32])
def test_schedule_helper_gives_the_steps_of_solve_master_equation(substeps):
    times, m, h = rafft_kin.kinetics_schedule(30, 100, substeps)
    assert np.array_equal(times, np.exp(np.arange(100) * (30 / 100) - 4))          # the reference's default spacing
    assert (m, h) == literal_schedule(times, substeps)
    assert m[0] == substeps and h[0] == times[0] / substeps
    times2, m2, h2 = rafft_kin.kinetics_schedule(sample_times=IRREGULAR, substeps=substeps)
    assert list(times2) == IRREGULAR and (m2, h2) == literal_schedule(IRREGULAR, substeps)
    for k in range(1, len(IRREGULAR)):                                             # every interval is covered exactly once
        assert math.isclose(m2[k] * h2[k], IRREGULAR[k] - IRREGULAR[k - 1], rel_tol=1e-15)


def test_solve_master_equation_takes_its_steps_from_the_helper(monkeypatch):
    """the integrator asks the helper, and its populations are those of the scheme written out with the literal schedule"""
    import torch
    calls = []
    real = rafft_kin.kinetics_schedule

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)

    monkeypatch.setattr(rafft_kin, "kinetics_schedule", spy)
    k01, k10 = 1.0, math.exp(-1.0 / 0.61)
    rate = np.array([[-k01, k01], [k10, -k10]])
    p0 = torch.tensor([1.0, 0.0], dtype=torch.float64)
    got = rafft_kin.solve_master_equation(torch.as_tensor(rate), [0.0, -1.0], p0, IRREGULAR, "implicit", 4)
    assert calls and all(c.get("substeps") == 4 for c in calls)
    A, y, want = rate.T, np.array([1.0, 0.0]), []
    g, c = 2.0 - 2.0 ** 0.5, 1.0 - 0.5 * 2.0 ** 0.5
    for m, h in zip(*literal_schedule(IRREGULAR, 4)):
        M = np.eye(2) - (c * h) * A
        for _ in range(m):
            yg = np.linalg.solve(M, y + (0.5 * g * h) * (A @ y))
            y = np.linalg.solve(M, yg / (g * (2.0 - g)) - ((1.0 - g) ** 2 / (g * (2.0 - g))) * y)
        want.append(y / y.sum())
    assert np.abs(got - np.stack(want)).max() < 1e-13


def test_kin_graph_record_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "rafft_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*rafft_kin_graph;", hdr).group(1)
    fields = re.findall(r"\b(int32_t|int64_t|double)\s+(\w+);", body)
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    assert [(name, ctype[t]) for t, name in fields] == list(_native.KinGraph._fields_)
    assert [name for _, name in fields][:5] == ["status", "n_rows", "row0", "n_unique", "n_edges"]
    assert ctypes.sizeof(_native.KinGraph) == 24
    cap = int(re.search(r"#define RAFFT_KIN_BATCH_MAX_STATES (\d+)", hdr).group(1))
    assert cap == _native.KIN_BATCH_MAX_STATES and 128 < cap <= 2048
    assert "rafft_kin_batch" in _native.EXPORTS
    proto = re.search(r"int rafft_kin_batch\(([^;]*)\);", hdr).group(1)
    assert len(proto.split(",")) == len(_native.lib().rafft_kin_batch.argtypes)


def test_cli_parses_kin():
    a = cli.parse_arguments(["-sf", "seqs.fa", "--batch", "--kin", "pops.txt"])
    assert (a.kin, a.max_time, a.n_steps) == ("pops.txt", 30, 100)                  # rafft_kin's defaults
    a = cli.parse_arguments(["-sf", "seqs.fa", "--batch", "--kin", "pops.txt", "-mt", "12.5", "-ns", "7"])
    assert (a.kin, a.max_time, a.n_steps) == ("pops.txt", 12.5, 7)
    assert cli.parse_arguments(["-s", "GGGAAACCC"]).kin is None


def test_cli_kin_writes_one_block_per_sequence(tmp_path):
    """the option's plumbing with the fold and the solver injected: a trajectory fold, one `> index sequence` block per sequence,
    rows sorted by final population in rafft_kin's format"""
    from rafft_amd.utils import Structure
    fa = tmp_path / "s.fa"
    fa.write_text(">a\nGGGAAACCC\n>b\nGGGGAAAACCCC\n")
    seen = {}

    def fold(seqs, *a):
        seen["traj"] = a[5]
        return [([Structure("." * len(s), 0)], [[Structure("." * len(s), 0)], [Structure("(" + "." * (len(s) - 2) + ")", -120)]]) for s in seqs]

    def solver(graphs, max_time, n_steps):
        seen["args"] = (max_time, n_steps)
        return [(None, None, None, [(g[0][0].str_struct, 0.0, 0.25, 0), (g[1][0].str_struct, -1.2, 0.75, 1)]) for g in graphs]

    out = tmp_path / "k.txt"
    cli.main(["-sf", str(fa), "--batch", "--kin", str(out), "-ns", "5"], fold_batch=fold, kinetics=solver)
    assert seen == {"traj": True, "args": (30, 5)}
    assert out.read_text().splitlines() == ["> 0 GGGAAACCC", ".........  0.250   0.0 0", "(.......)  0.750  -1.2 1",
                                            "> 1 GGGGAAAACCCC", "............  0.250   0.0 0", "(..........)  0.750  -1.2 1"]
    with pytest.raises(SystemExit):
        cli.main(["-s", "GGGAAACCC", "--kin", str(out)], fold_batch=fold, kinetics=solver)
