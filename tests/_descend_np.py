"""The gradient walk of rafft_descend_batch, restated for its tests (test infrastructure; pure Python: no GPU, no product code).

* `neighbours(seq, row)`: every neighbour of a structure under insertion and deletion of one pair, from a brute-force scan over all
  position pairs: (i, j, row') with the pair removed or - both positions unpaired, j - i > 3, a canonical pair of bases, no present
  pair crossing it - added.
* `walk(seq, row, max_steps, energy)`: the walk DESIGN.md section 14 defines - among the neighbours with dE < 0 the smallest
  (dE, i, j); none: the end - over WHOLE-STRUCTURE energies (`energy(seq, row)`, oracle.eval_structure by default): deliberately not
  incremental, so an error in the device's loop bookkeeping cannot hide in it.
* `parse_status(seq, row)`: what the library's host side must say of a start row.
* `starts()`: the fixed list of (sequence, start row) both test files use, with the conditions it must meet; `stats(walks)`.
"""
import numpy as np

import oracle
import _mfe_np as MF

CANONICAL = {"AU", "UA", "GC", "CG", "GU", "UG"}
ERR_STRUCT, ERR_CAPACITY = 8, 5


def pairs_of(row):
    stack, out = [], []
    for x, c in enumerate(row):
        if c == "(":
            stack.append(x)
        elif c == ")":
            out.append((stack.pop(), x))
    assert not stack
    return sorted(out)


def parse_status(seq, row):
    """0, or ERR_STRUCT for a row of another length than the sequence, a character outside ( ) . , an unbalanced row, a non-canonical
    pair or a hairpin of fewer than 3"""
    if len(row) != len(seq) or set(row) - set("()."):
        return ERR_STRUCT
    depth = 0
    for c in row:
        depth += (c == "(") - (c == ")")
        if depth < 0:
            return ERR_STRUCT
    if depth:
        return ERR_STRUCT
    pairs = pairs_of(row)
    for i, j in pairs:
        if seq[i] + seq[j] not in CANONICAL:
            return ERR_STRUCT
        if j - i - 1 < 3 and not any(i < p < j for p, _ in pairs):
            return ERR_STRUCT
    return 0


def neighbours(seq, row):
    """[(i, j, is_removal, new row)] in no particular order"""
    L, pairs = len(row), pairs_of(row)
    out = []
    for i, j in pairs:
        out.append((i, j, True, row[:i] + "." + row[i + 1:j] + "." + row[j + 1:]))
    for i in range(L):
        for j in range(i + 4, L):
            if row[i] != "." or row[j] != "." or seq[i] + seq[j] not in CANONICAL:
                continue
            if any((p < i < q < j) or (i < p < j < q) for p, q in pairs):
                continue
            out.append((i, j, False, row[:i] + "(" + row[i + 1:j] + ")" + row[j + 1:]))
    return out


# ---- neighbours, stated another way: two unpaired positions may pair when the same pair encloses both (they are members of one loop)

def move_row(row, i, j, rem):
    return row[:i] + ("." if rem else "(") + row[i + 1:j] + ("." if rem else ")") + row[j + 1:]


def all_neighbours(seq, row):
    """[(i, j, is_removal)], sorted"""
    out, members, stack = [], {}, [-1]
    for x, c in enumerate(row):
        if c == "(":
            stack.append(x)
        elif c == ")":
            out.append((stack.pop(), x, True))
        else:
            members.setdefault(stack[-1], []).append(x)
    for g in members.values():
        for a, i in enumerate(g):
            for j in g[a + 1:]:
                if j - i > 3 and seq[i] + seq[j] in CANONICAL:
                    out.append((i, j, False))
    return sorted(out)


def random_row(rng, seq, n_add):
    """the open chain of `seq` with up to n_add random legal pairs added, one after the other"""
    row = "." * len(seq)
    for _ in range(n_add):
        adds = [n for n in all_neighbours(seq, row) if not n[2]]
        if not adds:
            break
        i, j, _ = adds[int(rng.integers(len(adds)))]
        row = move_row(row, i, j, False)
    return row


# the lengths at which the lanes' stride over the positions, x = lane, lane + 64, ..., turns over
STRIDE_LENGTHS = (63, 64, 65, 129)


def stride_rows(L):
    """(seq, rows): a random sequence of L nt and four rows of it - the open chain, a few pairs, some helices' worth, and as many
    pairs as random additions find room for"""
    rng = np.random.default_rng(L)
    seq = "".join(rng.choice(list("ACGU"), L))
    return seq, [random_row(rng, seq, n) for n in (0, 3, L // 6, L)]


def walk(seq, row, max_steps=0, energy=oracle.eval_structure):
    """dict(status, end, n_steps, start_dcal, end_dcal, moves, dcal, ties, tie_kinds): moves as the library reports them - (i, j) for
    an added pair, (-i-1, -j-1) for a removed one; dcal: the energy of every row of the path; ties: the steps at which more than one
    neighbour had the lowest dE, tie_kinds: those of them at which a removal and an addition were among the tied"""
    bound = max_steps if max_steps > 0 else 2 * len(seq) + 16
    e = energy(seq, row)
    out = dict(status=0, n_steps=0, start_dcal=e, moves=[], dcal=[e], ties=0, tie_kinds=0)
    while True:
        cand = [(energy(seq, new) - e, i, j, rem, new) for i, j, rem, new in neighbours(seq, row)]
        cand = [c for c in cand if c[0] < 0]
        if not cand:
            break
        if out["n_steps"] == bound:
            out["status"] = ERR_CAPACITY
            break
        best = min(cand)
        tied = [c for c in cand if c[0] == best[0]]
        out["ties"] += len(tied) > 1
        out["tie_kinds"] += len({c[3] for c in tied}) > 1
        dE, i, j, rem, row = best
        e += dE
        out["moves"].append((-i - 1, -j - 1) if rem else (i, j))
        out["dcal"].append(e)
        out["n_steps"] += 1
    out.update(end=row, end_dcal=e)
    return out


def cached_energy(energy=oracle.eval_structure):
    cache = {}

    def en(seq, row):
        k = (seq, row)
        if k not in cache:
            cache[k] = energy(seq, row)
        return cache[k]
    return en


SEED = 20261021
_STARTS = []


def start_sequences(n=8, seed=SEED):
    """the first n random 16-22-nt sequences whose enumeration (canonical pairs, hairpins of at least 3) has 8 to 1000 structures,
    with their enumerations"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        seq = "".join(rng.choice(list("ACGU"), int(rng.integers(16, 23))))
        rows = MF.enumerate_structures(seq)
        if 8 <= len(rows) <= 1000:
            out.append((seq, rows))
    return out


def starts():
    """[(seq, row)]: every structure of the enumerations of start_sequences()"""
    if not _STARTS:
        _STARTS.extend((seq, row) for seq, rows in start_sequences() for row in rows)
    return _STARTS


def stats(walks):
    return dict(walks=len(walks), steps=sum(w["n_steps"] for w in walks), longest=max(w["n_steps"] for w in walks),
                zero=sum(w["n_steps"] == 0 for w in walks), ties=sum(w["ties"] for w in walks), tie_kinds=sum(w["tie_kinds"] for w in walks),
                both_kinds=sum(len({m[0] < 0 for m in w["moves"]}) == 2 for w in walks))


def check_conditions(st):
    """the conditions the list of starts must meet for the tests on it to say something"""
    assert st["ties"] >= 50 and st["tie_kinds"] >= 10 and st["both_kinds"] >= 200 and st["zero"] >= 50, st


_WALKS = {}


def mirror_walks(which="builtin"):
    """the walks of starts() under the tables that are installed (`which` names them for the cache), computed once"""
    if which not in _WALKS:
        en = cached_energy()
        _WALKS[which] = [walk(seq, row, 0, en) for seq, row in starts()]
        if which == "builtin":
            check_conditions(stats(_WALKS[which]))
    return _WALKS[which]
