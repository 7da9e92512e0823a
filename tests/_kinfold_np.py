"""The trajectories of rafft_kinfold_batch, restated for their tests (test infrastructure; pure Python: no GPU; of the product only
the exported weight table, which the table test checks against the formula).

* `philox(key, ctr)`: Philox4x32-10, restated (test_kinfold_host checks it against hostcheck/rng_check.cpp).
* `Mirror(W)`: the process DESIGN.md section 16 defines, under the tables that are installed when its energies are first asked for.
  Neighbours come from `_descend_np.neighbours`, dE from differences of WHOLE-STRUCTURE energies (oracle.eval_structure) -
  deliberately not incremental -, weights from the table W, the time step from math.log.  `trajectory(...)` returns what the
  library reports of one trajectory, and `near`: how many sample times lie within relative 1e-9 of a jump (there the last place of
  the device's logarithm may decide the record; the tests' grids are chosen so that this is 0).
* `generator(seq, rows, W)`: the generator matrix of the master equation over a full enumeration, from the same weights; rows that
  differ by one pair are neighbours.  `propagate(Q, p0, times)`: expm(Q t) p0.
"""
import math

import numpy as np

import oracle
import _descend_np as DS

KF_TIME, KF_STOP, KF_ABSORBED, KF_MORE = 1, 2, 4, 8
ERR_CAPACITY = 5
NW = 4096
DEFAULT_STEPS = 1 << 20
INVALID = (-2 ** 31, -2)
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85                     # the published constants
MASK = 0xFFFFFFFF
GAS = 1.98717e-3


def philox(key, ctr):
    k0, k1 = key
    c0, c1, c2, c3 = ctr
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def formula_weights(kT):
    """the table as the header states it, in Python floats"""
    return [1 << 32] + [int(math.floor(4294967296.0 * math.exp(-d / (100.0 * kT)) + 0.5)) for d in range(1, NW)]


def weight(W, dE):
    return int(W[0]) if dE <= 0 else int(W[dE]) if dE < NW else 0


class Mirror:
    def __init__(self, W, energy=oracle.eval_structure):
        self.W = [int(w) for w in W]
        self.energy = DS.cached_energy(energy)
        self._moves = {}

    def moves(self, seq, row):
        """the neighbours of a row in ascending (i, j): (i, j, is_removal, new row, dE, weight)"""
        key = (seq, row)
        if key not in self._moves:
            e = self.energy(seq, row)
            out = []
            for i, j, rem, new in sorted(DS.neighbours(seq, row), key=lambda c: (c[0], c[1])):
                dE = self.energy(seq, new) - e
                out.append((i, j, rem, new, dE, weight(self.W, dE)))
            self._moves[key] = out
        return self._moves[key]

    def trajectory(self, seq, row, k, seed, t_max, max_steps=0, watch=(), n_stop=0, grid=()):
        """dict(status, flags, n_steps, start_dcal, end_dcal, stop_index, time, end, moves, times, dcal, samples, wtot, near)"""
        watch = list(watch)
        bound = max_steps if max_steps > 0 else DEFAULT_STEPS
        widx = lambda r: watch.index(r) if r in watch else -1
        e = self.energy(seq, row)
        out = dict(start_dcal=e, moves=[], times=[], dcal=[e], samples=[], wtot=[], stop_index=-1)
        flags, steps, time, ti, drawn = 0, 0, 0.0, 0, []
        if row in watch[:n_stop]:
            flags, out["stop_index"] = KF_STOP, watch.index(row)
        while not flags:
            cand = self.moves(seq, row)
            wtot = sum(c[5] for c in cand)
            if wtot == 0:
                flags = KF_ABSORBED
                break
            o = philox((seed & MASK, seed >> 32), (k, steps, 0, 0))
            u = float((o[0] << 32 | o[1]) >> 11) * 2.0 ** -53
            v = o[2] << 32 | o[3]
            T = time + -math.log(1.0 - u) * 4294967296.0 / float(wtot)
            drawn.append(T)
            if T > t_max:
                flags = KF_TIME
                break
            while ti < len(grid) and grid[ti] < T:
                out["samples"].append((e, widx(row)))
                ti += 1
            if steps == bound:
                flags = KF_MORE
                break
            r = (v * wtot) >> 64
            acc = 0
            for i, j, rem, new, dE, w in cand:
                acc += w
                if acc > r:
                    break
            else:
                raise AssertionError("the drawn number met no move")
            out["wtot"].append(wtot)
            out["moves"].append((-i - 1, -j - 1) if rem else (i, j))
            out["times"].append(T)
            row, e, time, steps = new, e + dE, T, steps + 1
            assert e == self.energy(seq, row)
            out["dcal"].append(e)
            if row in watch[:n_stop]:
                flags, out["stop_index"] = KF_STOP, watch.index(row)
        while ti < len(grid):
            out["samples"].append(INVALID if flags & KF_MORE else (e, widx(row)))
            ti += 1
        near = sum(1 for tau in grid for T in drawn if abs(T - tau) <= 1e-9 * max(abs(tau), abs(T)))
        out.update(status=ERR_CAPACITY if flags & KF_MORE else 0, flags=flags, n_steps=steps, end=row, end_dcal=e,
                   time=t_max if flags & (KF_TIME | KF_ABSORBED) else time, near=near)
        return out


def generator(seq, rows, W, energy=oracle.eval_structure):
    """(Q, dcal): Q[b, a] = the rate from row a to row b in units of the rate of a downhill move (weight / 2^32), columns sum to 0"""
    sets = [frozenset(DS.pairs_of(r)) for r in rows]
    index = {s: k for k, s in enumerate(sets)}
    en = [energy(seq, r) for r in rows]
    all_pairs = sorted({p for s in sets for p in s})
    n = len(rows)
    Q = np.zeros((n, n))
    for a, s in enumerate(sets):
        for p in all_pairs:
            b = index.get(s ^ {p})
            if b is not None:
                Q[b, a] = weight(W, en[b] - en[a]) / 4294967296.0
    Q -= np.diag(Q.sum(axis=0))
    return Q, en


def propagate(Q, p0, times):
    """expm(Q t) p0 for every t: scaling and squaring of a Taylor series in float64 (Q is small, its entries lie in [-n, 1]; with
    the column sum of Q t / 2^s below 1/2, 30 terms leave less than 2^-30 / 30! of the series)"""
    out = []
    for t in times:
        A = Q * t
        s = max(0, int(math.ceil(math.log2(max(np.abs(A).sum(axis=0).max(), 1e-300)))) + 1)
        A = A / 2.0 ** s
        E, term = np.eye(len(Q)), np.eye(len(Q))
        for m in range(1, 30):
            term = term @ A / m
            E = E + term
        for _ in range(s):
            E = E @ E
        out.append(E @ p0)
    return np.array(out)
