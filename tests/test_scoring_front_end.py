"""Accuracy scoring, the parts that need no GPU: the C-ABI surface (rafft_score_rows / rafft_score_result) and the
`rafft -sf FILE --batch --scores OUT.csv` front-end with the fold and the scorer injected (oracle fold, tests/_scoring_np)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _scoring_np
import oracle
from conftest import ROOT
from rafft_amd import _native, cli, scoring


def test_score_entry_points_are_declared_exported_and_sized(tmp_path):
    header = open(os.path.join(ROOT, "include", "rafft_hip.h")).read()
    for name in ("rafft_score_rows", "rafft_score_result"):
        assert f"int {name}(" in header and name in _native.EXPORTS
        getattr(_native.lib(), name)
    assert header.count("benchmark_results/scoring.py:76-94") >= 1
    assert scoring._row_dtype().itemsize == 20 and scoring._seq_dtype().itemsize == 64
    assert scoring._seq_dtype().fields["best"][1] == 24 and scoring._seq_dtype().fields["first"][1] == 44
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "rafft_hip.h"\n'
                   "_Static_assert(sizeof(rafft_score_row) == 20, \"row\");\n_Static_assert(sizeof(rafft_score_seq) == 64, \"seq\");\n"
                   "_Static_assert(offsetof(rafft_score_row, status) == 16, \"row.status\");\n"
                   "_Static_assert(offsetof(rafft_score_seq, pick_ppv) == 16 && offsetof(rafft_score_seq, best) == 24 "
                   "&& offsetof(rafft_score_seq, first) == 44, \"seq\");\n")
    subprocess.check_call(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_score_entry_points_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_native.RafftError) as e:
        scoring.score_rows_gpu([["(...)", "....."]], ["(...)"])
    assert e.value.code == _native.ERR_NO_DEVICE
    with pytest.raises(_native.RafftError) as e:
        scoring.best_of_gpu(["(...)"], "(...)")
    assert e.value.code == _native.ERR_NO_DEVICE
    lib = _native.lib()
    res = _native.Result(0, 0, None, None)               # an empty fold result
    seq_out = np.zeros(1, scoring._seq_dtype())
    assert lib.rafft_score_result(ctypes.byref(res), None, None, seq_out.ctypes.data_as(ctypes.c_void_p)) == _native.ERR_NO_DEVICE
    # arguments are looked at first, as in every entry point
    one = (ctypes.c_int * 1)
    args = lambda n, L, rows: (n, one(L), one(rows), (ctypes.c_char_p * 1)(b"."), one(L), (ctypes.c_char_p * 1)(b"."), None,
                               seq_out.ctypes.data_as(ctypes.c_void_p))
    assert lib.rafft_score_rows(*args(-1, 1, 1)) == _native.ERR_PARAM
    assert lib.rafft_score_rows(*args(1, 32768, 1)) == _native.ERR_PARAM
    assert lib.rafft_score_rows(*args(1, 1, -1)) == _native.ERR_PARAM
    assert lib.rafft_score_rows(*args(1, 1, 1)) == _native.ERR_NO_DEVICE


def _oracle_fold_batch(seqs, n_mode=100, max_stack=1, max_branch=100, min_hp=3, min_nrj=0.0, traj=False, temp=37.0,
                       gc=3.0, au=2.0, gu=1.0, **kw):
    return [oracle.fold(s, n_mode, max_stack, max_branch, min_hp, min_nrj, traj, temp, gc, au, gu) for s in seqs]


def _np_scorer(results, known):
    return _scoring_np.table([[x.str_struct for x in beam] for beam in results], known)


def _short_rows(bench_rows, n):
    rows = [r for r in bench_rows if len(r["seq"]) <= 130]
    return rows[::max(1, len(rows) // n)][:n]


def _expected_lines(rows, ms, select):
    beams = [[(x.str_struct, x.dcal) for x in oracle.fold(r["seq"], 100, ms, 1000)] for r in rows]
    return _scoring_np.table_lines([(r["seq"], r["known"], r["name"]) for r in rows], beams, select)


def test_scores_table_from_headerless_and_named_csv(tmp_path, bench_rows):
    """`--batch --scores` on the reference's headerless seq,struct,name file and on a CSV with a header and other column names:
    header line, one line per sequence in input order, column formats, --select energy = row 0, --select ppv = last `>=`"""
    rows = _short_rows(bench_rows, 20)
    assert len(rows) == 20
    plain = tmp_path / "benchmark_cleaned.csv"
    plain.write_text("".join(f"{r['seq']},{r['known']},{r['name']}\n" for r in rows))
    named = tmp_path / "named.csv"
    named.write_text("id,sequence,truth\n" + "".join(f"{r['name']},{r['seq']},{r['known']}\n" for r in rows))
    named_args = ["--csv_column", "sequence", "--known_column", "truth", "--name_column", "id"]
    differ = 0
    for select in ("ppv", "energy"):
        want = _expected_lines(rows, 6, select)
        for f, extra in ((plain, []), (named, named_args)):
            out = tmp_path / f"{select}_{f.name}"
            cli.main(["-sf", str(f), "--batch", "-ms", "6", "--scores", str(out), "--select", select] + extra,
                     fold_batch=_oracle_fold_batch, scorer=_np_scorer)
            got = out.read_text().splitlines()
            assert got == want, (select, f.name)
        if select == "ppv":
            differ = sum(a != b for a, b in zip(want, _expected_lines(rows, 6, "energy")))
    assert differ > 0                                    # the two selections are not the same table
    line = _expected_lines(rows, 6, "ppv")[1].split(",")
    assert "." in line[3] and float(line[3]) <= 0 and line[5] == repr(float(line[5])) and line[6] == repr(float(line[6]))
    # a header whose first column name is made of sequence letters is still a header
    odd = tmp_path / "odd.csv"
    odd.write_text("tag,seq,struct\n" + "".join(f"{r['name']},{r['seq']},{r['known']}\n" for r in rows[:3]))
    out = tmp_path / "odd_out.csv"
    cli.main(["-sf", str(odd), "--batch", "-ms", "6", "--scores", str(out), "--name_column", "tag"], fold_batch=_oracle_fold_batch, scorer=_np_scorer)
    assert out.read_text().splitlines() == _expected_lines(rows[:3], 6, "ppv")
    # a file without known structures cannot be scored
    ln = tmp_path / "lines.txt"
    ln.write_text("\n".join(r["seq"] for r in rows[:3]) + "\n")
    with pytest.raises(SystemExit):
        cli.main(["-sf", str(ln), "--batch", "--scores", str(tmp_path / "x.csv")], fold_batch=_oracle_fold_batch, scorer=_np_scorer)
    with pytest.raises(SystemExit):
        cli.main(["-sf", str(named), "--batch", "--scores", str(tmp_path / "x.csv")] + named_args[:2] + ["--known_column", "nope"],
                 fold_batch=_oracle_fold_batch, scorer=_np_scorer)


def test_plain_batch_reads_the_headerless_reference_file(tmp_path, bench_rows):
    """`bin/rafft -sf benchmark_cleaned_all_length.csv --batch --bench`: the reference's file has no header line"""
    rows = _short_rows(bench_rows, 20)[:4]
    plain = tmp_path / "benchmark_cleaned.csv"
    plain.write_text("".join(f"{r['seq'].replace('U', 'T') if k == 1 else r['seq']},{r['known']},{r['name']}\n" for k, r in enumerate(rows)))
    out = tmp_path / "rows.txt"
    cli.main(["-sf", str(plain), "--batch", "--bench", "-ms", "3", "-o", str(out)], fold_batch=_oracle_fold_batch)
    want = ""
    for r in rows:
        for x in oracle.fold(r["seq"], 100, 3, 1000):
            want += f"{r['seq']} {len(r['seq'])} {x.str_struct} {x.energy:6.1f} {x.str_struct.count('(')}\n"
    assert out.read_text() == want
