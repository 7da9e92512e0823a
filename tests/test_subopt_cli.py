"""`rafft --subopt DELTA` without a device: main(..., subopt_batch=stub) - the option surface, the fast-folding-graph text with one
step 0 that holds the band in the library's order, the score table, and the options it excludes.  No GPU."""
import numpy as np
import pytest

from rafft_amd import cli
from rafft_amd.utils import Structure, parse_rafft_output

EXCLUSIVE = "--subopt gives every structure of every sequence within an energy band: no --mfe, no --pf, no --sample, no --kin, no --traj"


def _stub(calls):
    def stub(seqs, delta, max_structs, temp):
        calls.append((list(seqs), delta, max_structs, temp))
        out = []
        for s in seqs:
            n = len(s)
            # an order a sort by text would not give: the library's order is kept
            out.append([Structure("." + "(" + "." * (n - 4) + ")" + ".", -120), Structure("(" + "." * (n - 2) + ")", -120), Structure("." * n, 0)])
        return out
    return stub


def test_cli_subopt_graph_text_scores_and_exclusions(tmp_path, capsys):
    calls = []
    stub = _stub(calls)
    a = cli.parse_arguments(["-s", "GGGAAACCC", "--subopt", "1.5", "--max-structs", "70"])
    assert a.subopt == 1.5 and a.max_structs == 70
    b = cli.parse_arguments(["-s", "GGGAAACCC"])
    assert b.subopt is None and b.max_structs == 100000
    cli.main(["-s", "GGGAAACCC", "--subopt", "1.5", "--max-structs", "70"], subopt_batch=stub)
    text = capsys.readouterr().out
    assert calls[-1] == (["GGGAAACCC"], 1.5, 70, 37.0)
    assert text.splitlines() == ["GGGAAACCC", "# " + "{:-^20}".format(0), ".(.....).   -1.2", "(.......)   -1.2", ".........    0.0"]
    out = tmp_path / "one.txt"
    cli.main(["-s", "GGGAAACCC", "--subopt", "0", "-o", str(out)], subopt_batch=stub)
    assert out.read_text() == text and calls[-1][1:] == (0.0, 100000, 37.0)
    steps, seq = parse_rafft_output(str(out))
    assert seq == "GGGAAACCC" and len(steps) == 1
    assert [(st.str_struct, st.dcal) for st in steps[0]] == [(".(.....).", -120), ("(.......)", -120), (".........", 0)]
    fa = tmp_path / "s.fa"
    fa.write_text(">a\nGGGAAACCC\n>b\nACGUACGU\n")
    out2 = tmp_path / "two.txt"
    cli.main(["-sf", str(fa), "--batch", "--subopt", "2", "-o", str(out2)], subopt_batch=stub)
    assert out2.read_text().splitlines() == ["GGGAAACCC", "# " + "{:-^20}".format(0), ".(.....).   -1.2", "(.......)   -1.2", ".........    0.0",
                                             "ACGUACGU", "# " + "{:-^20}".format(0), ".(....).   -1.2", "(......)   -1.2", "........    0.0"]
    assert calls[-1][0] == ["GGGAAACCC", "ACGUACGU"]
    # --scores: the band of a sequence is scored as a beam
    csvf = tmp_path / "k.csv"
    csvf.write_text("GGGAAACCC,((.....)),x1\nACGUACGU,........,x2\n")
    seen = {}

    def scorer(beams, known):
        seen["beams"], seen["known"] = [[st.str_struct for st in b] for b in beams], list(known)
        z = np.zeros(2, dtype=np.int32)
        return dict(pick_ppv=np.array([1, 0]), pick_first=z, row0=np.array([0, 3]), n_known=np.array([2, 0]), seq_status=z,
                    n_pred=np.array([1, 1, 0, 1, 1, 0]), hit_pred=np.array([1, 1, 0, 0, 0, 0]), hit_known=np.array([1, 1, 0, 0, 0, 0]))

    sc = tmp_path / "scores.csv"
    cli.main(["-sf", str(csvf), "--batch", "--subopt", "1", "--scores", str(sc)], subopt_batch=stub, scorer=scorer)
    assert seen == {"beams": [[".(.....).", "(.......)", "........."], [".(....).", "(......)", "........"]], "known": ["((.....))", "........"]}
    lines = sc.read_text().splitlines()
    assert lines[0] == "seq,len_seq,struct,nrj,nbp,pvv,sens,name" and len(lines) == 3
    assert lines[1].startswith("GGGAAACCC,9,") and lines[1].endswith(",x1") and lines[2].startswith("ACGUACGU,8,")
    for extra in (["--mfe"], ["--pf"], ["--sample", "3"], ["--traj"], ["--kin", str(tmp_path / "kin.txt")]):
        with pytest.raises(SystemExit) as e:
            cli.main(["-sf", str(fa), "--batch", "--subopt", "2"] + extra, subopt_batch=stub)
        assert str(e.value) == EXCLUSIVE
    with pytest.raises(SystemExit, match="0 kcal/mol or more"):
        cli.main(["-s", "GGGAAACCC", "--subopt", "-1"], subopt_batch=stub)
    with pytest.raises(SystemExit, match="positive number"):
        cli.main(["-s", "GGGAAACCC", "--subopt", "1", "--max-structs", "0"], subopt_batch=stub)
    with pytest.raises(SystemExit, match="--scores needs -sf CSV --batch"):
        cli.main(["-s", "GGGAAACCC", "--subopt", "2", "--scores", str(sc)], subopt_batch=stub)
