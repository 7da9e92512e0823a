"""The seam calls - the entry points that drain the folds in flight and borrow workspace 0 on the caller's thread
(rafft_amd/csrc/rafft_seam.h): they share one entry (SeamGuard) and one owner of their per-call device buffers (DevScratch).
Pinned here, on tiny inputs: the calls interleaved with folds give the same results every time, an error return releases
what the call held and the next call is unharmed, and rafft_expand_node's nested evaluation rescales the tables for its
temperature."""
import ctypes as C

import numpy as np
import pytest

import rafft_amd
import oracle
from rafft_amd import _native as N, landscape, params, rafft as R, rafft_kin, scoring
import _par_reader as PR
from test_gpu_params import synthetic      # noqa: F401  (fixture: the enthalpy-bearing parameter file of the parameter tests)

pytestmark = pytest.mark.gpu

SEQS = ["GGGUUUGCGGUGUAAGUGCAGCCCGUCUUACACCGUGCGGCACAGGCACUAGUACUGAUG", "GGGGAAAACCCCUUGGAAACAAGGCGAAAGCC", "GCGCGAUAUAUUUUAUAUAUCGCGC"]
KNOWN = ["(((...(((((((.(((.........))).)))))))...)))......<<<....>>>.", "((((....))))[[[[...]]]].........", "(((((((((((...)))))))))))"]
# a region behind a branch helix, inside a closing pair: the enclosing loop is (4, 34), its branch (5, 14)
NODE_SEQ = "GGCGC" + "GGGAAAUCCC" + "AA" + "GGAGCGAAAAGCUCC" + "AA" + "GCGCC"
NODE_DB = "(((((" + "(((....)))" + "." * 19 + ")))))"
NODE_POS = list(range(15, 34))


def traj_key(traj):
    return [[(x.str_struct, x.dcal) for x in st] for st in traj]


def table_key(t):
    return {k: np.asarray(v).tobytes() for k, v in t.items()}


def graph(traj):
    """(struct_list[:8], their energies, the flat arrays of the C-ABI) of a folding trajectory with beams of 8 at most"""
    assert max(len(st) for st in traj) <= 8
    sizes, rows, uid, energy, struct_list = rafft_kin.graph_arrays(traj)
    return [s.str_struct for s in struct_list][:8], energy[:8], (sizes, rows, uid, energy)


def kin_call(sizes, rows, uid, energy, L):
    import torch
    S = len(energy)
    rate = torch.full((S, S), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = N.lib().rafft_kin_rate_matrix(len(sizes), sizes.ctypes.data_as(C.POINTER(C.c_int)), L, rows, uid.ctypes.data_as(C.POINTER(C.c_int)), S,
                                       energy.ctypes.data_as(C.POINTER(C.c_double)), rafft_kin.KT, C.c_void_p(rate.data_ptr()))
    return rc, rate.cpu().numpy()


def dist_call(structs):
    import torch
    S, L = len(structs), len(structs[0])
    D = torch.zeros((S, S), dtype=torch.uint16, device="cuda")
    torch.cuda.synchronize()
    rc = N.lib().rafft_landscape_distances(S, L, "".join(structs).encode(), D.data_ptr())
    return rc, D.cpu().numpy()


def one_pass():
    out = {}
    res = rafft_amd.fold_batch(SEQS, 100, 8, 1000, traj=True)
    out["fold"] = [traj_key(t) for _, t in res]
    out["node"] = R.expand_node(NODE_SEQ, NODE_DB, NODE_POS, 50, 3, 0.0)         # its nested evaluation runs under the outer guard
    out["fold_again"] = [(x.str_struct, x.dcal) for x in rafft_amd.fold(SEQS[1], 100, 4, 1000)]
    finals = [res[k][0][0].str_struct for k in range(len(SEQS))]
    out["eval"] = R.eval_structures(SEQS + [NODE_SEQ], finals + [NODE_DB], temp=37.0)
    structs, energy, arrays = graph(res[0][1])
    rc, rate = kin_call(*arrays, len(SEQS[0]))
    assert rc == 0
    out["kin"] = rate.tobytes()
    D = landscape.distance_matrix_gpu(structs)
    out["dist"] = D.cpu().numpy().tobytes()
    pos, stress, n_iter, (X, stresses, n_iters) = landscape.mds_gpu(D, n_init=2, max_iter=20, eps=1e-9, random_state=3)
    out["mds"] = (X.tobytes(), stresses.tobytes(), n_iters.tobytes())
    ti, z = landscape.surface_gpu(pos, energy, grid=8)
    out["surface"] = (ti.tobytes(), z.tobytes())
    out["score_result"] = table_key(scoring.score_batch_gpu(res, KNOWN))
    out["score_rows"] = table_key(scoring.score_rows_gpu([[x.str_struct for x in res[k][0]] for k in range(len(SEQS))], KNOWN))
    assert len(structs) >= 3 and D.shape[0] == len(structs) <= 8 and sum(out["eval"][1]) == 0
    return out


def test_gpu_seam_calls_interleaved_with_folds_repeat_exactly():
    params.reset_params()
    first, second = one_pass(), one_pass()
    assert first.keys() == second.keys()
    for k in first:
        assert first[k] == second[k], k
    assert first["node"]["lag"] and first["node"]["ddcal"]                        # the region really has lags to rank


def test_gpu_seam_call_error_returns_release_and_recover():
    """each call that keeps its per-call buffers in the shared owner fails by an ordinary error return, then the valid call
    gives what it gave before.  (rafft_landscape_mds has no such return to provoke: its last pass, pass == max_iter, stops
    every start, so "did not finish within max_iter + 1 passes" cannot be reached with valid arguments.)"""
    params.reset_params()
    fin, traj = rafft_amd.fold(SEQS[0], 100, 8, 1000, traj=True)
    structs, energy, (sizes, rows, uid, en) = graph(traj)
    L = len(SEQS[0])
    bad_rows = b")" + rows[1:]
    rc, good = kin_call(sizes, rows, uid, en, L)
    assert rc == 0
    rc, _ = kin_call(sizes, bad_rows, uid, en, L)
    assert rc == N.ERR_STRUCT and b"malformed dot-bracket row" in N.lib().rafft_last_error()
    rc, again = kin_call(sizes, rows, uid, en, L)
    assert rc == 0 and again.tobytes() == good.tobytes()

    rc, good = dist_call(structs)
    assert rc == 0
    rc, _ = dist_call([")" + structs[0][1:]] + structs[1:])
    assert rc == N.ERR_STRUCT and b"malformed dot-bracket row" in N.lib().rafft_last_error()
    rc, again = dist_call(structs)
    assert rc == 0 and again.tobytes() == good.tobytes()

    lib = N.lib()
    n = 2
    a = (C.c_char_p * n)(SEQS[1].encode(), NODE_SEQ.encode())
    ok = (C.c_char_p * n)(b"((((....))))" + b"." * 20, NODE_DB.encode())
    bad = (C.c_char_p * n)(b"(" + b"." * 31, NODE_DB.encode())
    good, out = (C.c_int * n)(), (C.c_int * n)()
    assert lib.rafft_eval_structures_at(37.0, n, a, ok, good, None) == 0
    assert lib.rafft_eval_structures_at(37.0, n, a, bad, out, None) == N.ERR_STRUCT          # status_out null: an error code
    assert b"malformed structure" in lib.rafft_last_error()
    assert lib.rafft_eval_structures_at(37.0, n, a, ok, out, None) == 0 and list(out) == list(good)
    assert list(good) == R.eval_structures([SEQS[1], NODE_SEQ], [ok[0].decode(), NODE_DB])[0]


def expand_node_at(temp, seq, db, pos, nb_mode=50, min_hp=3):
    n = len(pos)
    K = max(1, min(nb_mode, 2 * n - 1))
    p = R._params(nb_mode, 1, 100, min_hp, 0.0, False, temp, 3.0, 2.0, 1.0)
    nr, nk = C.c_int(), C.c_int()
    I, D = (lambda: (C.c_int * K)()), (lambda: (C.c_double * K)())
    lag, cv, nb, mi, mj, sc, dd, kept = I(), D(), I(), I(), I(), D(), I(), I()
    N.check(N.lib().rafft_expand_node(C.byref(p), seq.encode(), db.encode(), (C.c_int * n)(*pos), n, C.byref(nr), lag, cv, nb, mi, mj, sc,
                                      dd, C.byref(nk), kept))
    return dict(lag=list(lag[:nr.value]), ddcal=list(dd[:nr.value]), kept=list(kept[:nk.value]))


def test_gpu_expand_node_rescales_the_tables_for_its_temperature(synthetic):
    """the evaluation nested in rafft_expand_node (under the outer guard) brings the device tables to p->temp: lags, dE and kept
    candidates equal what the CPU oracle gives with the tests' own rescaling of the same file (tests/_par_reader.py) - at 25 C
    with the tables at 37 C before the call, then at 37 C with them at 25 C.  The oracle stands in for the reference this case was
    meant to have, the ddcal of the parent commit's library on an MI355X as literals: those have not been taken."""
    path, par = synthetic
    params.load_params(path)
    want = {}
    for temp in (25.0, 37.0):
        oracle.set_tables(PR.tables_at(par, temp))
        o = oracle.expand_node(NODE_SEQ, NODE_DB, NODE_POS, 50, 3, 0.0, 3.0, 2.0, 1.0)
        want[temp] = dict(lag=o["lag"], ddcal=o["ddcal"], kept=o["kept"])
    dc37, st = R.eval_structures([NODE_SEQ], [NODE_DB], temp=37.0)               # the device tables are the file's at 37 C now
    at25 = expand_node_at(25.0, NODE_SEQ, NODE_DB, NODE_POS)                      # ... the nested evaluation brings them to 25 C
    at37 = expand_node_at(37.0, NODE_SEQ, NODE_DB, NODE_POS)                      # ... and back
    assert st == [0]
    assert at25 == want[25.0] and at37 == want[37.0]
    assert at25["kept"] and at25["ddcal"] != at37["ddcal"]                        # really other tables, and a stem they price
