"""rafft_pf_span_batch on a real MI355X (`-m gpu`): Z, every P(i,j) and every unpaired probability against the sums over every
structure of short sequences that obeys the span, against rafft_pf_batch where the span does not bind, against the tests' own mirror
where it does, on blocks between runs of N where the exterior windows start above 0 and where the sequence is far longer than any
mirror reaches, on a sequence whose exterior sums leave the fp64 range, at other temperatures, same input - same bits, errors that
stay with their sequence, and the command line.
The bounds are those of tests/test_gpu_pf.py: 1e-8 kcal/mol on the ensemble energy, 1e-9 on a probability and on an unpaired
probability, 1e-9 relative on the MFE's share.  Where a sequence is a concatenation of B independent blocks its energy is the sum of
B block energies, each held to 1e-8: the bound is B x 1e-8."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import rafft_amd
from rafft_amd import _native as N, mccaskill, params, rafft as R, zuker
from conftest import ROOT
import _loops as LP
import _par_reader as PR
import _pf_np as PF
import _pf_span_np as PS
from test_gpu_pf import enumerated, exhaustive_sequences, mirror_sequences, rand

pytestmark = pytest.mark.gpu

TABLES = ("builtin", "multiloops_win")
KT = PF.kt_of(37.0)
E_TOL, P_TOL, F_TOL = 1e-8, 1e-9, 1e-9


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    builtin = LP.builtin_par()
    idx = LP.index_sensitive_par(builtin)
    idx.update(ml_closing=-700, ml_intern=-300)
    out = dict(builtin=builtin, multiloops_win=idx, synthetic=PR.synthetic_par(builtin), paths={})
    d = tmp_path_factory.mktemp("par")
    for name, comment in (("multiloops_win", "index-sensitive, multiloops win"), ("synthetic", "made-up enthalpies")):
        out["paths"][name] = d / (name + ".par")
        PR.write_par(out[name], out["paths"][name], comment=comment)
    return out


def install(sets, which):
    if which == "builtin":
        params.reset_params()
    else:
        params.load_params(sets["paths"][which])


@pytest.fixture(autouse=True)
def back_to_builtin():
    yield
    params.reset_params()


def bits(rows, recs, probs, un, k):
    """everything rafft_pf_span_batch returns for sequence k, as bytes and integers"""
    r = recs[k]
    return (rows[k], r["status"], r["mfe_dcal"], r["n_pairs"], np.float64(r["energy"]).tobytes(), np.float64(r["mfe_frequency"]).tobytes(),
            None if probs is None or probs[k] is None else probs[k].tobytes(), None if un is None or un[k] is None else un[k].tobytes())


def centroid_of(P):
    db = ["."] * P.shape[0]
    for a, b in zip(*np.nonzero(P > 0.5)):
        db[a], db[b] = "(", ")"
    return "".join(db)


# ---- 0. the symbol

def test_gpu_pf_span_symbol_and_record():
    assert N.lib().rafft_pf_span_batch is not None
    rows, recs, probs, un = mccaskill.pf_span_batch_raw(["GGGGAAAACCCC"], 40)
    assert rows == ["((((....))))"] and recs[0]["status"] == 0 and recs[0]["length"] == 12 and recs[0]["n_pairs"] == 4
    assert recs[0]["energy"] < recs[0]["mfe_dcal"] / 100.0 < 0 and 0.5 < recs[0]["mfe_frequency"] < 1.0
    assert probs[0].shape == (12, 12) and probs[0][0, 11] > 0.5 and un[0][5] > 0.9 and un[0][0] < 0.5
    res = rafft_amd.pf_span("GGGGAAAACCCC", 8)
    assert res.probs.shape == (12, 8) and res.unpaired.shape == (12,) and res.centroid.count("(") <= 2


# ---- 1. every structure that obeys the span

@pytest.mark.parametrize("which", TABLES)
def test_gpu_pf_span_equals_the_sums_over_every_structure_that_obeys_the_span(sets, which):
    install(sets, which)
    seqs = exhaustive_sequences()
    assert 40 <= len(seqs) <= 59 and max(map(len, seqs)) == 20 and sum("N" in s for s in seqs) == 5
    rows = enumerated(seqs)
    en, st = R.eval_structures([s for s, rr in zip(seqs, rows) for _ in rr], [r for rr in rows for r in rr])      # one call
    assert not any(st)
    wanted = [sorted({1, 4, 5, 6, 8, 12, max(len(s) - 1, 1), len(s), 4096}) for s in seqs]
    got = {span: mccaskill.pf_span_batch_raw(seqs, span) for span in sorted(set().union(*wanted))}
    mfe = {span: zuker.mfe_span_batch_raw(seqs, span)[1] for span in got}
    worst_e = worst_p = worst_f = worst_u = 0.0
    at = n_bound = 0
    for k, (s, rr) in enumerate(zip(seqs, rows)):
        L = len(s)
        e = en[at:at + len(rr)]
        at += len(rr)
        w = [math.exp(-x / (100.0 * KT)) for x in e]
        prs = [PF.pairs_of(r) for r in rr]
        reach = [max((j - i + 1 for i, j in p), default=0) for p in prs]
        for span in wanted[k]:
            _, recs, probs, un = got[span]
            keep = [x for x in range(len(rr)) if reach[x] <= span]
            Z = math.fsum(w[x] for x in keep)
            per = {}
            for x in keep:
                for ij in prs[x]:
                    per.setdefault(ij, []).append(w[x])
            P = np.zeros((L, L))
            for (i, j), xs in per.items():
                P[i, j] = math.fsum(xs) / Z
            r = recs[k]
            assert r["status"] == 0 and r["mfe_dcal"] == min(e[x] for x in keep) == mfe[span][k], (s, span)
            dense = mccaskill.band_to_dense(probs[k])
            assert probs[k].shape == (L, min(L, span))
            worst_e = max(worst_e, abs(r["energy"] - (-KT * math.log(Z))))
            worst_p = max(worst_p, float(np.abs(dense - P).max()))
            worst_u = max(worst_u, float(np.abs(un[k] - PS.unpaired_of(P)).max()))
            worst_f = max(worst_f, abs(r["mfe_frequency"] / (math.exp(-r["mfe_dcal"] / (100.0 * KT)) / Z) - 1.0))
            n_bound += len(keep) < len(rr)
            if span <= 4 or L <= 4:
                assert r["energy"] == 0.0 and r["mfe_frequency"] == 1.0 and not probs[k].any() and (un[k] == 1.0).all() and got[span][0][k] == "." * L
    print(f"\n{which}: largest error of the energy {worst_e:.3g} kcal/mol, of P {worst_p:.3g}, of unpaired {worst_u:.3g}, of the MFE share {worst_f:.3g} (relative); "
          f"the span excludes structures in {n_bound} cases")
    assert worst_e <= E_TOL and worst_p <= P_TOL and worst_u <= P_TOL and worst_f <= F_TOL
    assert n_bound >= 100


# ---- 2. span >= L against rafft_pf_batch

def test_gpu_pf_span_at_least_the_length_equals_pf_batch():
    rng = np.random.default_rng(19)
    seqs = mirror_sequences() + [rand(rng, n) for n in (150, 300, 530, 700, 1200)]
    rows0, recs0, probs0 = mccaskill.pf_batch_raw(seqs)
    assert not any(r["status"] for r in recs0)
    worst_e = worst_p = worst_f = worst_u = 0.0
    got = mccaskill.pf_span_batch_raw(seqs, 4096)
    rows, recs, probs, un = got
    for k, s in enumerate(seqs):
        r = recs[k]
        assert r["status"] == 0 and r["mfe_dcal"] == recs0[k]["mfe_dcal"] and probs[k].shape == (len(s), len(s))
        dense = mccaskill.band_to_dense(probs[k])
        worst_e = max(worst_e, abs(r["energy"] - recs0[k]["energy"]))
        worst_p = max(worst_p, float(np.abs(dense - probs0[k]).max()))
        worst_u = max(worst_u, float(np.abs(un[k] - PS.unpaired_of(probs0[k])).max()))
        worst_f = max(worst_f, abs(r["mfe_frequency"] / recs0[k]["mfe_frequency"] - 1.0))
        close = np.abs(probs0[k] - 0.5) <= P_TOL                                   # a pair that near 0.5 may fall on either side
        assert rows[k] == rows0[k] or close.any()
        assert r["n_pairs"] == rows[k].count("(")
        assert bits(*mccaskill.pf_span_batch_raw([s], len(s)), 0) == bits(*got, k)  # span = L: the same band, the same bits
    print(f"\nspan >= L against rafft_pf_batch: largest difference of the energy {worst_e:.3g} kcal/mol, of P {worst_p:.3g}, of unpaired {worst_u:.3g}, "
          f"of the MFE share {worst_f:.3g} (relative)")
    # the share is exp((energy - mfe) / kT): two energies 1e-8 kcal/mol apart give shares E_TOL / kT = 1.6e-8 apart, relatively
    assert worst_e <= E_TOL and worst_p <= P_TOL and worst_u <= P_TOL and worst_f <= E_TOL / KT


# ---- 3. the mirror where the span binds

# closing helix, a stem, 51 unpaired bases, a stem: in the cell M[5][83] the last stem starts at 70 = 5 + 65, candidate 64 of the
# split - lane 0 in its second round
ML65 = "GGGGC" + "GCGCG" + "GAAA" + "CGCGC" + "A" * 51 + "GGCCG" + "GAAA" + "CGGCC" + "GCCCC"


def binding_sequences():
    rng = np.random.default_rng(5)
    seqs = [rand(rng, n) for n in (60, 101, 150)] + [ML65]
    for run in (30, 31):
        seqs.append("GGGCG" + "A" * run + "GCGCG" + "GAAA" + "CGCGC" + "CGCCC")
    return seqs


_MIRROR = {}


def mirrored(sets, which, span, s, temp=37.0):
    key = (which, span, s, temp)
    if key not in _MIRROR:
        _MIRROR[key] = PS.PfSpanMirror(PR.tables_at(sets[which], temp), span, temp).run(s)
    return _MIRROR[key]


def against_mirror(seqs, got, mir, kt):
    """largest errors of the energy, P, unpaired against [(Z, P, unpaired)]; the centroid rows are the mirror's"""
    rows, recs, probs, un = got
    worst_e = worst_p = worst_u = 0.0
    for k, (Z, P, U) in enumerate(mir):
        assert recs[k]["status"] == 0
        worst_e = max(worst_e, abs(recs[k]["energy"] - (-kt * math.log(Z))))
        worst_p = max(worst_p, float(np.abs(mccaskill.band_to_dense(probs[k]) - P).max()))
        worst_u = max(worst_u, float(np.abs(un[k] - U).max()))
        if not (np.abs(P - 0.5) <= P_TOL).any():
            assert rows[k] == centroid_of(P) and recs[k]["n_pairs"] == rows[k].count("(")
    return worst_e, worst_p, worst_u


@pytest.mark.parametrize("span", [10, 30, 64, 65, 100])
def test_gpu_pf_span_equals_the_mirror_where_the_span_binds(sets, span):
    seqs = binding_sequences()
    assert len(ML65) == 89 and [len(s) for s in seqs[-2:]] == [54, 55]
    got = mccaskill.pf_span_batch_raw(seqs, span)
    worst = against_mirror(seqs, got, [mirrored(sets, "builtin", span, s) for s in seqs], KT)
    print(f"\nspan {span}: largest error of the energy {worst[0]:.3g} kcal/mol, of P {worst[1]:.3g}, of unpaired {worst[2]:.3g}")
    assert worst[0] <= E_TOL and worst[1] <= P_TOL and worst[2] <= P_TOL
    free = mccaskill.pf_batch_raw(seqs)
    dense = [mccaskill.band_to_dense(p) for p in got[2]]
    if span <= 65:                                                                 # the span binds on the 150 nt: structures are lost
        assert got[1][2]["energy"] > free[1][2]["energy"] + 1e-3
    k = seqs.index(ML65)
    if span == 100:
        assert dense[k][4, 84] > 0.9                                               # the multiloop with the stem at candidate 64
        install(sets, "multiloops_win")
        win = mccaskill.pf_span_batch_raw([ML65], span)
        worst = against_mirror([ML65], win, [mirrored(sets, "multiloops_win", span, ML65)], KT)
        print(f"multiloops_win: largest error of the energy {worst[0]:.3g} kcal/mol, of P {worst[1]:.3g}, of unpaired {worst[2]:.3g}")
        assert worst[0] <= E_TOL and worst[1] <= P_TOL and worst[2] <= P_TOL
        assert mccaskill.band_to_dense(win[2][0])[0, 88] > 0.1
    else:
        assert not dense[k][4, 84]
    # the interior-loop cap: over the bulge of 30 the outer helix (4, L - 5), 46 positions, is nearly certain once the span lets it
    # form, over 31 it is nearly absent
    p30, p31 = dense[-2][4, 49], dense[-1][4, 50]
    assert (p30 > 0.99 if span >= 46 else p30 == 0.0) and p31 < 0.01


# ---- 4. windows that start above 0

def helix_block(rng, n):
    return "GGGCGC" + rand(rng, n - 12) + "GCGCCC"


@pytest.mark.parametrize("size, gap", [(140, 150), (280, 300), (560, 600)])
def test_gpu_pf_span_blocks_between_runs_of_n(size, gap):
    rng = np.random.default_rng(size)
    blocks = [helix_block(rng, size + dx) for dx in (0, -3, 5, 2)]
    whole = ("N" * gap).join(blocks)
    span = gap
    assert span >= max(map(len, blocks)) and len(whole) > 3 * span
    flanked = [("N" if k else "") + b + ("N" if k < 3 else "") for k, b in enumerate(blocks)]
    rows0, recs0, probs0 = mccaskill.pf_batch_raw(flanked)
    rows, recs, probs, un = mccaskill.pf_span_batch_raw([whole], span)
    assert recs[0]["status"] == 0 and not any(r["status"] for r in recs0) and probs[0].shape == (len(whole), span)
    e_sum = math.fsum(r["energy"] for r in recs0)
    print(f"\n{len(whole)} nt, span {span}: energy {recs[0]['energy']:.6f} against the blocks' sum {e_sum:.6f} kcal/mol")
    assert abs(recs[0]["energy"] - e_sum) <= 4 * E_TOL
    assert recs[0]["mfe_dcal"] == sum(r["mfe_dcal"] for r in recs0)
    at, worst_p, worst_u = 0, 0.0, 0.0
    want_row = ""
    covered = np.zeros(len(whole), dtype=bool)
    for k, b in enumerate(blocks):
        lead = 1 if k else 0
        Pb = probs0[k][lead:lead + len(b), lead:lead + len(b)]
        band = probs[0][at:at + len(b)]
        worst_p = max(worst_p, float(np.abs(band - PS.dense_to_band(Pb, span)).max()))
        worst_u = max(worst_u, float(np.abs(un[0][at:at + len(b)] - PS.unpaired_of(Pb)).max()))
        covered[at:at + len(b)] = True
        want_row += rows0[k][lead:lead + len(b)] + ("." * gap if k < 3 else "")
        at += len(b) + gap
    print(f"largest difference of P {worst_p:.3g}, of unpaired {worst_u:.3g}")
    assert worst_p <= P_TOL and worst_u <= P_TOL
    assert not probs[0][~covered].any() and (un[0][~covered] == 1.0).all()         # block-diagonal; every N unpaired
    assert rows[0] == want_row and recs[0]["n_pairs"] == want_row.count("(") > 0


# ---- 5. long sequences

def gc_blocks():
    rng = np.random.default_rng(55)
    return [rand(rng, n, "ACGU", [0.15, 0.35, 0.35, 0.15]) for n in (55, 58, 61, 63, 65)]


def tiled(L, blocks, gap=70, lead_only=False):
    """a sequence of exactly L: a run of N, then blocks in turn between runs of `gap` N, the last block ending at L - 1; the offsets
    and numbers of the blocks"""
    parts, where, n, k = [], [], 0, 0
    while True:
        b = blocks[k % len(blocks)]
        if n + len(b) + gap > L - 1 and parts:
            break
        parts.append(b)
        where.append(k % len(blocks))
        n += len(b) + gap
        k += 1
    n -= gap                                                                       # no run behind the last block
    lead = L - n
    assert lead >= 1
    text, offs, at = "N" * lead, [], lead
    for x, b in enumerate(parts):
        offs.append(at)
        text += b + ("N" * gap if x + 1 < len(parts) else "")
        at += len(b) + gap
    assert len(text) == L
    return text, offs, where


def block_mirror(sets, span, b, right=True):
    """the mirror of block b behind an N (and before one): (energy, P over the block, unpaired over the block, centroid)"""
    Z, P, U = mirrored(sets, "builtin", span, "N" + b + ("N" if right else ""))
    Pb = P[1:1 + len(b), 1:1 + len(b)]
    return -KT * math.log(Z), Pb, U[1:1 + len(b)], centroid_of(Pb)


def check_tiled(sets, span, text, offs, where, blocks, got, k=0, last_open=True):
    """sequence k of `got` is `text`: its energy is the sum of the blocks' mirror energies, P inside each block, unpaired and the
    centroid are the mirror's, everything else is unpaired; returns the number of blocks"""
    rows, recs, probs, un = got
    L, W = len(text), min(span, len(text))
    assert recs[k]["status"] == 0 and probs[k].shape == (L, W)
    e_sum, want_row, at_end = 0.0, ["."] * L, 0
    covered = np.zeros(L, dtype=bool)
    worst_p = worst_u = 0.0
    for x, (o, w) in enumerate(zip(offs, where)):
        b = blocks[w]
        e, Pb, Ub, cen = block_mirror(sets, span, b, right=not (last_open and x + 1 == len(offs)))
        e_sum += e
        worst_p = max(worst_p, float(np.abs(probs[k][o:o + len(b)] - PS.dense_to_band(Pb, W)).max()))
        worst_u = max(worst_u, float(np.abs(un[k][o:o + len(b)] - Ub).max()))
        covered[o:o + len(b)] = True
        want_row[o:o + len(b)] = cen
    B = len(offs)
    print(f"\n{L} nt, span {span}, {B} blocks: energy {recs[k]['energy']:.6f} against the mirror's sum {e_sum:.6f} kcal/mol; largest difference of P {worst_p:.3g}, "
          f"of unpaired {worst_u:.3g}")
    assert abs(recs[k]["energy"] - e_sum) <= B * E_TOL
    assert worst_p <= P_TOL and worst_u <= P_TOL
    assert not probs[k][~covered].any() and (un[k][~covered] == 1.0).all()
    assert rows[k] == "".join(want_row) and recs[k]["n_pairs"] == rows[k].count("(")
    return B


@pytest.mark.parametrize("span", [40, 70])
def test_gpu_pf_span_long_sequences(sets, span):
    blocks = gc_blocks()
    cases = [tiled(L, blocks) for L in (4097, 17000, N.MFE_SPAN_MAX_LEN)]
    nine = "GGGAAACCC"
    seqs = [c[0] for c in cases] + ["A" * (N.MFE_SPAN_MAX_LEN + 1), nine]
    got = mccaskill.pf_span_batch_raw(seqs, span)
    assert [r["status"] for r in got[1]] == [0, 0, 0, N.ERR_TOO_LONG, 0]
    assert N.lib().rafft_last_error().decode() == "sequence 3: longer than RAFFT_MFE_SPAN_MAX_LEN"
    assert got[0][3] == "." * (N.MFE_SPAN_MAX_LEN + 1) and got[1][3]["energy"] == 0.0 and got[2][3] is None
    for k, (text, offs, where) in enumerate(cases):
        B = check_tiled(sets, span, text, offs, where, blocks, got, k)
        assert B >= len(text) // 140
    # the last pair of the longest: the last block ends at position 32767
    text, offs, where = cases[2]
    last = blocks[where[-1]]
    _, Pb, _, cen = block_mirror(sets, span, last, right=False)
    i, j = max(zip(*np.nonzero(Pb)), key=lambda ij: (ij[1], -ij[0]))
    assert offs[-1] + len(last) == N.MFE_SPAN_MAX_LEN and j == len(last) - 1
    assert abs(got[2][2][offs[-1] + i, j - i] - Pb[i, j]) <= P_TOL and Pb[i, j] > 0.0
    alone = mccaskill.pf_span_batch_raw([nine], span)
    assert bits(*got, 4) == bits(*alone, 0) and got[0][4] == "(((...)))"


# ---- 6. the range of the exterior sums

@pytest.mark.parametrize("n_first", [True, False])
def test_gpu_pf_span_exterior_sums_beyond_the_fp64_range(sets, n_first):
    """half of the sequence is N, half GC-rich blocks: under the one scale of the sequence the exterior sum decays (or grows) by
    |ln scale| per N, over the N half by more than 745 = -ln(the smallest fp64): a plain fp64 F is 0 (or inf) at its end"""
    span, half = 70, 8192
    blocks = gc_blocks()
    text, offs, where = tiled(half, blocks)
    lead = len(text) - len(text.lstrip("N"))
    if n_first:
        seq, offs2 = "N" * half + text, [o + half for o in offs]
    else:                                                                          # the blocks first, behind one N: the rest of the run that led them follows them
        seq, offs2 = text[lead - 1:] + "N" * (half + lead - 1), [o - lead + 1 for o in offs]
    assert len(seq) == 2 * half
    e_blocks = math.fsum(block_mirror(sets, span, blocks[w], right=not (n_first and x + 1 == len(offs)))[0] for x, w in enumerate(where))
    mfe = zuker.mfe_span_batch_raw([seq], span)[1][0]
    ln_scale = -1.07 * (mfe / 100.0) / (KT * len(seq))
    print(f"\n{len(seq)} nt: span MFE {mfe} dcal/mol, ensemble energy of the blocks {e_blocks:.3f} kcal/mol, ln scale {ln_scale:.4f}: {ln_scale * half:.0f} over the N half")
    assert abs(ln_scale) * half > 745.0
    got = mccaskill.pf_span_batch_raw([seq], span)
    assert got[1][0]["status"] == 0 and got[1][0]["mfe_dcal"] == mfe
    check_tiled(sets, span, seq, offs2, where, blocks, got, 0, last_open=n_first)
    n_half = slice(0, half) if n_first else slice(half - lead + 1, 2 * half)
    assert (got[3][0][n_half] == 1.0).all() and not got[2][0][n_half].any()


# ---- 7. other temperatures

@pytest.mark.parametrize("temp", [25.0, 60.0])
def test_gpu_pf_span_at_another_temperature(sets, temp):
    install(sets, "synthetic")
    seqs, span = binding_sequences()[:2] + [ML65], 30
    at37 = mccaskill.pf_span_batch_raw(seqs, span)
    got = mccaskill.pf_span_batch_raw(seqs, span, temp=temp)
    kt = PF.kt_of(temp)
    worst = against_mirror(seqs, got, [mirrored(sets, "synthetic", span, s, temp) for s in seqs], kt)
    print(f"\n{temp} C, span {span}: largest error of the energy {worst[0]:.3g} kcal/mol, of P {worst[1]:.3g}, of unpaired {worst[2]:.3g}")
    assert worst[0] <= E_TOL and worst[1] <= P_TOL and worst[2] <= P_TOL
    shift = [abs(a["energy"] - b["energy"]) for a, b in zip(got[1], at37[1])]
    assert min(shift) > 1e5 * E_TOL                                                # kT and every table moved
    again = mccaskill.pf_span_batch_raw(seqs, span)
    assert [bits(*again, k) for k in range(len(seqs))] == [bits(*at37, k) for k in range(len(seqs))]


# ---- 8. same input, same bits

def test_gpu_pf_span_same_input_same_bits():
    rng = np.random.default_rng(6)
    seqs = [rand(rng, n) for n in (33, 58, 171, 20, 64, 45, 80, 9)]
    span = 50
    whole = mccaskill.pf_span_batch_raw(seqs, span)
    assert not any(r["status"] for r in whole[1])
    want = {s: bits(*whole, k) for k, s in enumerate(seqs)}
    for k in (0, 3, len(seqs) - 1):                                                # alone
        assert bits(*mccaskill.pf_span_batch_raw([seqs[k]], span), 0) == want[seqs[k]]
    for order in (seqs[::-1], [seqs[k] for k in rng.permutation(len(seqs))], seqs[1:] + seqs[:1]):
        got = mccaskill.pf_span_batch_raw(order, span)
        assert [bits(*got, k) for k in range(len(order))] == [want[s] for s in order]
    # several chunks: room for the tables of two 64-nt sequences, then one sequence a chunk
    for budget in (2 * 6 * 64 * 50 * 8, 1):
        got = mccaskill.pf_span_batch_raw(seqs, span, workspace_bytes=budget)
        assert [bits(*got, k) for k in range(len(seqs))] == [want[s] for s in seqs]
    rows2, recs2, none, none2 = mccaskill.pf_span_batch_raw(seqs, span, probs=False, unpaired=False)
    assert none is None and none2 is None and rows2 == whole[0] and recs2 == whole[1]


# ---- 9. errors stay with their sequence

def test_gpu_pf_span_reports_a_sequence_whose_band_cells_leave_the_fp64_range():
    rng = np.random.default_rng(404)
    big, left, right = "G" * 200 + "GAAA" + "C" * 200, rand(rng, 40), rand(rng, 25)
    seqs = [left, big, right]
    mfe = zuker.mfe_span_batch_raw([big], 4096)[1][0]
    assert mfe < -60000
    for sf in (1e-9, 3.0):
        without = mccaskill.pf_span_batch_raw([left, right], 4096, scale_factor=sf)
        assert not any(x["status"] for x in without[1])
        rows, recs, probs, un = mccaskill.pf_span_batch_raw(seqs, 4096, scale_factor=sf)
        r = recs[1]
        assert [x["status"] for x in recs] == [0, N.ERR_CAPACITY, 0], sf
        assert N.lib().rafft_last_error().decode().startswith("sequence 1:")
        assert rows[1] == "." * len(big) and r["energy"] == 0.0 and r["mfe_frequency"] == 0.0 and r["n_pairs"] == 0 and r["length"] == len(big)
        assert r["mfe_dcal"] == mfe
        assert probs[1].shape == (len(big), len(big)) and not probs[1].any() and not un[1].any()
        assert [bits(rows, recs, probs, un, 0), bits(rows, recs, probs, un, 2)] == [bits(*without, 0), bits(*without, 1)]
    without = mccaskill.pf_span_batch_raw([left, right], 4096)
    rows, recs, probs, un = mccaskill.pf_span_batch_raw(seqs, 4096)
    r, ref = recs[1], mccaskill.pf_batch_raw([big])
    assert r["status"] == N.OK and r["mfe_dcal"] == mfe and abs(r["energy"] - ref[1][0]["energy"]) <= E_TOL
    assert np.abs(mccaskill.band_to_dense(probs[1]) - ref[2][0]).max() <= P_TOL and rows[1] == ref[0][0]
    assert [bits(rows, recs, probs, un, 0), bits(rows, recs, probs, un, 2)] == [bits(*without, 0), bits(*without, 1)]


def test_gpu_pf_span_errors_stay_with_their_sequence():
    good = ["GGGGAAAACCCC", "GGGAAACCCAGGGAAACCC", "GCGCUUCGGCGC", "ACGUACGUACGUACGUAGC"]
    span = 12
    alone = mccaskill.pf_span_batch_raw(good, span)
    seqs = [good[0], "", good[1], "GGGXAAACCC", good[2], "A" * (N.MFE_SPAN_MAX_LEN + 1), good[3]]
    rows, recs, probs, un = mccaskill.pf_span_batch_raw(seqs, span)                 # returns: the call is RAFFT_OK
    assert [r["status"] for r in recs] == [0, N.ERR_EMPTY, 0, N.ERR_BAD_CHAR, 0, N.ERR_TOO_LONG, 0]
    assert N.lib().rafft_last_error().decode().startswith("sequence 1")
    assert [rows[k] for k in (1, 3, 5)] == ["", "." * 10, "." * (N.MFE_SPAN_MAX_LEN + 1)]
    assert all(recs[k]["energy"] == 0.0 and recs[k]["n_pairs"] == 0 and recs[k]["mfe_frequency"] == 0.0 for k in (1, 3, 5))
    assert not probs[3].any() and not un[3].any() and probs[5] is None and un[5] is None
    assert [bits(rows, recs, probs, un, k) for k in (0, 2, 4, 6)] == [bits(*alone, k) for k in range(4)]
    got = rafft_amd.pf_span_batch(seqs, span, raise_errors=False)
    assert [g is None for g in got] == [False, True, False, True, False, True, False]
    assert got[0].centroid == rows[0] and got[0].energy == recs[0]["energy"] and got[0].mfe_energy == recs[0]["mfe_dcal"] / 100.0
    assert np.array_equal(got[0].probs, probs[0]) and np.array_equal(got[0].unpaired, un[0]) and rafft_amd.pf_span(good[0], span, probs=False).probs is None
    with pytest.raises(KeyError):
        rafft_amd.pf_span_batch(seqs[2:4], span)
    # RAFFT_ERR_PARAM: the outputs are not touched, and the next call is exact
    L = N.lib()
    buf = ctypes.create_string_buffer(b"untouched!", 16)
    out = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    rec = (N.PfSeq * 1)()
    rec[0].status, rec[0].energy = 77, 7.5
    pr, uu = np.full((12, 12), 3.25), np.full(12, 2.5)
    pp, up = (ctypes.c_void_p * 1)(pr.ctypes.data), (ctypes.c_void_p * 1)(uu.ctypes.data)
    seq = (ctypes.c_char_p * 1)(good[0].encode())
    ln = (ctypes.c_int * 1)(12)
    for args in ((-1, seq, ln, 37.0, 0.0, span, 0, rec, out, pp, up), (1, None, ln, 37.0, 0.0, span, 0, rec, out, pp, up), (1, seq, ln, 37.0, 0.0, span, 0, None, out, pp, up),
                 (1, seq, ln, 37.0, -0.5, span, 0, rec, out, pp, up), (1, seq, ln, 37.0, float("nan"), span, 0, rec, out, pp, up),
                 (1, seq, ln, 37.0, float("inf"), span, 0, rec, out, pp, up), (1, seq, ln, 37.0, 0.0, span, -1, rec, out, pp, up),
                 (1, seq, ln, 37.0, 0.0, 0, 0, rec, out, pp, up), (1, seq, ln, 37.0, 0.0, -3, 0, rec, out, pp, up), (1, seq, ln, 37.0, 0.0, 4097, 0, rec, out, pp, up)):
        assert L.rafft_pf_span_batch(*args) == N.ERR_PARAM
        assert buf.value == b"untouched!" and rec[0].status == 77 and rec[0].energy == 7.5 and (pr == 3.25).all() and (uu == 2.5).all()
    assert bits(*mccaskill.pf_span_batch_raw(good[:1], span), 0) == bits(*alone, 0)
    for batch in (good, ["", "GGGXAACCC"]):                                        # the built-in tables are 37 C only, as for the fold
        with pytest.raises(N.RafftError) as e:
            mccaskill.pf_span_batch_raw(batch, span, temp=25.0)
        assert e.value.code == N.ERR_TEMP


# ---- 10. the command line as a process

def test_gpu_cli_pf_span(tmp_path):
    from rafft_amd import cli
    rng = np.random.default_rng(10)
    rows = [(helix_block(rng, 70), "x1"), (rand(rng, 120), "x2"), ("GGGAAACCC", "x3")]
    known = ["." * len(s) for s, _ in rows]
    csvf = tmp_path / "known.csv"
    csvf.write_text("".join(f"{s},{k},{n}\n" for (s, n), k in zip(rows, known)))
    out, lines, bpp = tmp_path / "scores.csv", tmp_path / "lines.txt", tmp_path / "bpp.txt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "rafft"), "-sf", str(csvf), "--batch", "--pf", "--pf-span", "40", "--scores", str(out), "-o", str(lines),
                        "--bpp", str(bpp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    want = rafft_amd.pf_span_batch([s for s, _ in rows], 40)
    free = rafft_amd.pf_batch([s for s, _ in rows], probs=False)
    assert lines.read_text().splitlines() == [cli.format_pf_line(s, res) for (s, _), res in zip(rows, want)]
    assert want[0].energy > free[0].energy + 1e-3                                  # the span was passed on: the closing helix is lost
    got = out.read_text().splitlines()
    assert got[0] == "seq,len_seq,struct,nrj,nbp,pvv,sens,name" and len(got) == 1 + len(rows)
    for line, (s, name), res in zip(got[1:], rows, want):
        assert line.startswith(f"{s},{len(s)},{res.centroid},{res.energy},{res.centroid.count('(')},") and line.endswith("," + name)
    text = bpp.read_text().splitlines()
    expect = [f"{name} {i + 1} {j + 1} {p:.6g}" for (s, name), res in zip(rows, want) for i, j, p in mccaskill.band_pairs(res.probs, 1e-5)]
    assert text == expect and len(text) > 20 and all(int(t.split()[2]) - int(t.split()[1]) + 1 <= 40 for t in text)
