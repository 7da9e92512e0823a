"""bench.py's own surface: a plain run (the headline line only), `--full` for the rest, and `--dump-outputs DIR` - the final
beams of the last timed step as .npy files, the same for every build of the same inputs."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _result(N, seqs, beams):
    """a rafft_result as the library hands it out: per sequence `length + 1` bytes per structure (NUL-terminated rows)"""
    keep = []
    srs = (N.SeqResult * len(seqs))()
    for i, (s, (status, rows)) in enumerate(zip(seqs, beams)):
        raw = b"".join(r.encode() + b"\0" for r in rows)
        db = C.create_string_buffer(raw, len(raw) + 1)
        dcal = (C.c_int32 * max(1, len(rows)))(*[-130 * (k + 1) for k in range(len(rows))])
        keep += [db, dcal]
        srs[i].status, srs[i].length, srs[i].n_structs = status, len(s), len(rows)
        srs[i].db, srs[i].dcal = C.cast(db, C.POINTER(C.c_char)), C.cast(dcal, C.POINTER(C.c_int32))
    res = N.Result(len(seqs), sum(1 for st, _ in beams if st), C.cast(srs, C.POINTER(N.SeqResult)), None)
    return C.pointer(res), keep


def test_dump_outputs_of_a_result(tmp_path):
    from rafft_amd import _native as N
    seqs = ["GGGAAACCC", "ACGUACGU", "GGGGAAAACCCC"]
    beams = [(0, ["(((...)))", ".........", "((.....))"]), (1, []), (0, ["((((....))))"])]
    res, keep = _result(N, seqs, beams)
    recs = bench.beam_records(res, len(seqs))
    assert [r[0] for r in recs] == [0, 1, 0] and [len(r[1]) for r in recs] == [3, 0, 1]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), recs, [len(s) for s in seqs], 50)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == ["dcal", "n_pairs", "n_structs", "status", "structures_sample", "structures_sample_seq"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["status"].tolist() == [0, 1, 0] and got["n_structs"].tolist() == [3, 0, 1]
    assert got["dcal"].tolist() == [-130, -260, -390, -130] and got["n_pairs"].tolist() == [3, 0, 2, 4]
    # three short sequences: all of them in the sample, every structure as '.' 0, '(' 1, ')' 2
    assert got["structures_sample_seq"].tolist() == [0, 1, 2]
    want = "".join(beams[0][1] + beams[2][1])
    assert got["structures_sample"].tolist() == [".()".index(c) for c in want]
    for name, a in got.items():       # the same result dumps the same files
        assert np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy")))


def test_dump_of_full_beams_is_bounded_and_samples_by_length(tmp_path):
    """the benchmark set with every beam of ms=50 full: the dump stays below 64 MB, and the sampled sequences depend on the
    lengths alone (two different outputs of the same inputs sample the same sequences)"""
    lengths = [len(s) for s in bench.load_bench_sequences()]
    picks = []
    for d, ch in (("a", "."), ("b", "(")):
        recs = [(0, np.zeros(50, np.int32), np.full((50, L), ord(ch), np.uint8)) for L in lengths]
        bench.dump_outputs(str(tmp_path / d), recs, lengths, 50)
        files = [tmp_path / d / f for f in os.listdir(tmp_path / d)]
        assert sum(f.stat().st_size for f in files) <= 64e6
        picks.append(np.load(tmp_path / d / "structures_sample_seq.npy").tolist())
        assert np.load(tmp_path / d / "structures_sample.npy").size == 50 * sum(lengths[int(i)] for i in picks[-1])
    assert picks[0] == picks[1] and len(picks[0]) > len(lengths) // 2


def test_bench_arguments():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


def _check_dump(out, copies):
    """the dump of a step that folded `copies` copies of the benchmark set == the Python API's fold of the set, copy after copy"""
    import rafft_amd
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sum(a.nbytes for a in got.values()) <= 64e6
    seqs = bench.load_bench_sequences()
    want = list(rafft_amd.fold_batch(seqs, 100, 50, 1000)) * copies
    assert got["status"].tolist() == [0] * len(want)
    assert got["n_structs"].tolist() == [len(fin) for fin in want]
    assert got["dcal"].tolist() == [x.dcal for fin in want for x in fin]
    assert got["n_pairs"].tolist() == [x.str_struct.count("(") for fin in want for x in fin]
    pick = [int(i) for i in got["structures_sample_seq"]]
    assert len(pick) > len(seqs) // 2
    assert got["structures_sample"].tolist() == [".()".index(c) for i in pick for x in want[i] for c in x.str_struct]


def _line(r):
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_gpu_bench_plain_run_dumps_the_last_step(tmp_path):
    """a plain run prints the headline line without the --full figures, and its dump is the fold of the benchmark set that the
    Python API returns for the same parameters"""
    out = tmp_path / "dump"
    line = _line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                                 "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600))
    assert line["unit"] == "sequences/s" and line["higher_is_better"] is True and line["steps"] == 3 and line["n_gpus"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["metric"] and line["dtype"]
    assert abs(line["value"] - 2296 * 1e3 / line["ms_per_step"]) < 1e-3 * line["value"]
    assert line["cpu_baseline"] is None and line["parity_vs_cpu"] is None and line["python_api"] is None
    assert "steady_state_value" not in line and line["stage_ms_untimed_pass"] is None
    _check_dump(out, 1)


@pytest.mark.gpu
def test_gpu_bench_two_ranks_dump_the_whole_step(tmp_path):
    """--gpus 2 (two ranks on the one GPU, gloo): rank 0 gathers every rank's shard of the last step in the order of the step's
    global batch - two copies of the set"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(BENCH_SAME_GPU="1", BENCH_BACKEND="gloo")
    out = tmp_path / "dump"
    line = _line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                                 "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=600))
    assert line["n_gpus"] == 2 and line["steps"] == 2 and "strong_value" not in line
    _check_dump(out, 2)
