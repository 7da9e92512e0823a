"""Constructed fast-folding graphs for the kinetics rate matrix, and an independent reference of it.

Nothing here imports the library or its host mirror.  `reference_rate_matrix` restates the reference's
`get_connected_prev` / `get_transition_mat` (rafft/rafft_kin.py:48-56, 68-91) literally: Python sets of (i, j) pairs from a
stack parse, `pairs_prev - pairs_cur == set()`, `fast_paths[step_i - 1]` with Python's negative index, the energy of a
structure's first appearance.  The rate argument is formed in IEEE double as the reference forms it, its exponential is
taken with mpmath at 60 digits and rounded once to double, the diagonal is minus the exactly rounded row sum.

The builders return lists of steps of `Row`s (`str_struct`, `energy`), the shape `utils.parse_rafft_output` gives.  Any
well-nested dot-bracket is a legal row, `()` included: the kernels know no hairpin rule."""
import math

import mpmath
import numpy as np

KT = 0.61
LENGTH_EDGES = (1, 2, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 4097, 32767)
STAR_SIZES = (1, 2, 255, 256, 257, 513)
ENERGY_STEPS = (0.0, 0.1, 1e-9, 100.0, 440.0, 460.0, 5000.0)      # 440 > 709 * 0.61 (exp overflows), 460 > 745 * 0.61 (underflows to 0)
ENERGY_KTS = (0.61, 0.2, 5.0)
FACING_SIZES = (1, 2, 3, 4, 5, 9, 1, 9, 5, 4, 3, 2, 1)            # every n_prev of {1, 2, 3, 4, 5, 9} faces a smaller and a larger step


class Row:
    __slots__ = ("str_struct", "energy")

    def __init__(self, str_struct, energy):
        self.str_struct = str_struct
        self.energy = energy

    def __repr__(self):
        return f"Row({self.str_struct!r}, {self.energy!r})"


# ---------------------------------------------------------------- the reference

def parse_pairs(db):
    """(i, j) pairs of a dot-bracket row from a stack parse; ValueError on anything but a well-nested row of ( ) ."""
    stack, pairs = [], []
    for x, c in enumerate(db):
        if c == "(":
            stack.append(x)
        elif c == ")":
            if not stack:
                raise ValueError(f"unmatched ) at {x}")
            pairs.append((stack.pop(), x))
        elif c != ".":
            raise ValueError(f"foreign character {c!r} at {x}")
    if stack:
        raise ValueError(f"unmatched ( at {stack[-1]}")
    return pairs


def unique_rows(fast_paths):
    """rows in order of first appearance (rafft_kin.py:106-112) and their index by string"""
    index, ordered = {}, []
    for step in fast_paths:
        for st in step:
            if st.str_struct not in index:
                index[st.str_struct] = len(ordered)
                ordered.append(st)
    return ordered, index


_TINY = mpmath.mpf(2) ** -1074          # the smallest double subnormal
_NORMAL = mpmath.mpf(2) ** -1022


def metropolis(arg):
    """min(1, exp(arg)) for a double `arg`, the exponential exact to 60 digits, rounded once to double"""
    if arg >= 0.0:
        return 1.0                      # exp(arg) >= 1, +inf included
    with mpmath.workdps(60):
        e = mpmath.exp(mpmath.mpf(arg))
        if e < _TINY:
            return 0.0
        if e < _NORMAL:                 # a subnormal result: round to a whole number of 2^-1074 (no second rounding)
            return math.ldexp(int(mpmath.nint(e / _TINY)), -1074)
        return float(e)


def reference_rate_matrix(fast_paths, kt=KT):
    ordered, index = unique_rows(fast_paths)
    struct_map = {st.str_struct: (index[st.str_struct], st.energy) for st in ordered}
    pair_sets = {}

    def pairs_of(db):
        if db not in pair_sets:
            pair_sets[db] = set(parse_pairs(db))
        return pair_sets[db]

    S = len(ordered)
    entries = {}
    rates = {}
    for step_i, fold_step in enumerate(fast_paths):
        prev_step = fast_paths[step_i - 1]
        for struct in fold_step:
            pairs_cur = pairs_of(struct.str_struct)
            map_cur, cur_nrj = struct_map[struct.str_struct]
            for prev_st in prev_step:
                if pairs_of(prev_st.str_struct) - pairs_cur:
                    continue
                map_prev, prev_nrj = struct_map[prev_st.str_struct]
                delta_nrj = float(cur_nrj) - float(prev_nrj)
                if map_cur != map_prev:
                    for key, arg in (((map_prev, map_cur), -delta_nrj / kt), ((map_cur, map_prev), delta_nrj / kt)):
                        if arg not in rates:
                            rates[arg] = metropolis(arg)
                        entries[key] = rates[arg]
    mat = np.zeros((S, S), dtype=np.float64)
    by_row = [[] for _ in range(S)]
    for (r, c), v in entries.items():
        mat[r, c] = v
        by_row[r].append(v)
    for r in range(S):
        mat[r, r] = -math.fsum(by_row[r])
    return mat


def parse_graph_text(path):
    """the fast-folding-graph text of `rafft --traj` (a sequence line, `# --` step headers, `structure energy` rows)"""
    steps = []
    with open(path) as fh:
        fh.readline()
        for line in fh:
            if line.startswith("# --"):
                steps.append([])
            else:
                db, nrj = line.split()
                steps[-1].append(Row(db, float(nrj)))
    return steps


# ---------------------------------------------------------------- builders

def db_of(L, pairs):
    """dot-bracket row with `pairs`; None when they cross, share a position or leave the row"""
    s = ["."] * L
    for i, j in pairs:
        if not (0 <= i < j < L) or s[i] != "." or s[j] != ".":
            return None
        s[i], s[j] = "(", ")"
    db = "".join(s)
    return db if sorted(parse_pairs(db)) == sorted(pairs) else None


def length_edge_graph(L, max_children=None):
    """Step 0: the unfolded row.  Step 1: five parents = a base pair (8, 20) + one special pair each.  Step 2: for every
    parent a superset (which misses exactly the special pair of each OTHER parent: a near-superset of those) and, where
    the row has room, the parent with its special pair re-partnered (same left end, another right end); the base alone
    + one pair (a near-superset of all five); all compatible specials at once; two rows without the base pair.
    The special pairs, with c the start of the last 64-chunk: both ends in chunk 0; ends on both sides of the last
    64-boundary; the last two positions; both ends in the last chunk short of its end (or, when the last chunk is too
    short, L-3, L-2 re-partnered to L-1); a pair of chunk 0 that is re-partnered."""
    unfolded = Row("." * L, 0.0)
    if L < 63:
        rows = [Row(db, e) for db, e in {1: [(".", 0.0)], 2: [("()", -1.3), ("..", 0.0)]}[L]]
        return [[unfolded], rows, rows[::-1]]
    c = (L - 1) // 64 * 64
    base = (8, 20)
    extra = (45, 50)
    specials = [((1, 5), (1, 6))]                                            # (pair, its re-partnering or None)
    if c >= 64:
        hi = min(c + 1, L - 1)
        specials.append(((c - 2, hi), (c - 2, hi - 1) if hi - 1 >= c else (c - 2, c - 1)))
    else:
        specials.append(((22, 28), (22, 27)))                                # one chunk only: nothing to straddle
    specials.append(((L - 2, L - 1), None))
    if L - 3 > max(c, L - 6):
        specials.append(((max(c, L - 6), L - 3), (max(c, L - 6), L - 2)))
    else:
        specials.append(((L - 3, L - 2), (L - 3, L - 1)))
    specials.append(((30, 40), (30, 44)))
    parents = [Row(db_of(L, [base, sp]), -1.0 - 0.3 * k) for k, (sp, _) in enumerate(specials)]
    children = [(f"sup{k}", db_of(L, [base, sp, extra])) for k, (sp, _) in enumerate(specials)]
    children += [(f"rep{k}", db_of(L, [base, rep])) for k, (_, rep) in enumerate(specials) if rep is not None]
    children.append(("near_all", db_of(L, [base, extra])))
    both = [base, extra]
    for sp, _ in specials:
        if db_of(L, both + [sp]) is not None:
            both.append(sp)
    children.append(("all", db_of(L, both)))
    children.append(("no_base", db_of(L, [extra])))
    children.append(("other_base", db_of(L, [(9, 19), extra])))
    taken = {p.str_struct for p in parents}
    children = [(lab, db) for lab, db in children if db not in taken]     # (a re-partnering that is another parent)
    assert None not in taken and all(db is not None for _, db in children), L
    assert len(taken) == 5 and len({db for _, db in children}) == len(children), L
    if max_children is not None:             # the tail cases first
        order = ["sup2", "rep3", "near_all", "all", "sup1", "no_base"]
        children = [ch for ch in children if ch[0] in order[:max_children]]
    children = [db for _, db in children]
    step2 = [Row(db, -3.0 - 0.1 * k) for k, db in enumerate(children)]
    return [[unfolded], parents, step2]


def length_edge_graphs():
    return [(f"L{L}", length_edge_graph(L, 6 if L == 32767 else None), KT) for L in LENGTH_EDGES]


def _nested(L, k):
    """k pairs (0, L-1), (1, L-2), ..."""
    return db_of(L, [(i, L - 1 - i) for i in range(k)])


def facing_graph(sizes=FACING_SIZES, L=128, seed=20):
    """Steps of the given sizes.  Rows are sets of the slots (2i, 2i+1).  Row r of a step holds the slots of row
    (n_prev - 1 - r) mod n_prev of the step before, so the LAST row of every step has a child, + one new slot; every third
    row then loses one inherited slot (a near-superset)."""
    rng = np.random.default_rng(seed)
    n_slots = L // 2
    prev_sets = None
    steps = []
    for s, n in enumerate(sizes):
        cur_sets = []
        for r in range(n):
            if prev_sets is None:
                slots = set()
            else:
                slots = set(prev_sets[(len(prev_sets) - 1 - r) % len(prev_sets)])
                free = [x for x in range(n_slots) if x not in slots]
                slots.add(int(rng.choice(free)))
                if r % 3 == 2 and len(slots) > 1:
                    slots.discard(sorted(slots)[int(rng.integers(len(slots)))])
            cur_sets.append(slots)
        steps.append([Row(db_of(L, [(2 * x, 2 * x + 1) for x in sorted(sl)]), -1.0 * s - 0.07 * r) for r, sl in enumerate(cur_sets)])
        prev_sets = cur_sets
    return steps


def step_shape_graphs():
    L = 70
    unf = "." * L
    a, ab, abc = _nested(L, 1), _nested(L, 2), _nested(L, 3)
    return [
        # one step: it is compared with itself (fast_paths[0 - 1]), which connects the nested rows
        ("single_step", [[Row(a, -1.0), Row(ab, -2.5), Row(abc, -2.0)]], KT),
        # the unfolded row again in the last step: step 0 meets it there, equal uid, nothing written
        ("unfolded_in_last", [[Row(unf, 0.0)], [Row(a, -1.0)], [Row(ab, -2.5), Row(unf, 0.0)]], KT),
        # an empty step in the middle (the step after it has no predecessors) and one at the end (neither has step 0)
        ("empty_steps", [[Row(unf, 0.0)], [Row(a, -1.0)], [], [Row(ab, -2.5)], []], KT),
        # folded rows in step 0 and their subsets in the last step: only the negative index connects them
        ("last_into_first", [[Row(abc, -2.0), Row(a, -1.0)], [Row(ab, -2.5)], [Row(unf, 0.0), Row(a, -1.0)]], KT),
        ("facing", facing_graph(), KT),
    ]


def duplicate_graphs():
    L = 70
    unf = "." * L
    a, ab, abc = _nested(L, 1), _nested(L, 2), _nested(L, 3)
    b = db_of(L, [(30, 40)])
    return [
        ("twice_in_one_step", [[Row(unf, 0.0)], [Row(a, -1.0), Row(a, -1.0), Row(b, -0.4)], [Row(ab, -2.5)]], KT),
        ("in_three_steps", [[Row(unf, 0.0)], [Row(a, -1.0)], [Row(a, -1.0), Row(ab, -2.5)], [Row(a, -1.0), Row(abc, -2.0)]], KT),
        # the later appearances carry other energies, as current and as previous row: the first one counts
        ("other_energy_later", [[Row(unf, 0.0)], [Row(a, -1.0)], [Row(a, -7.0), Row(ab, -2.5)],
                                [Row(ab, 3.0), Row(a, 3.0), Row(abc, -2.0)], [Row(abc, -9.0), Row(unf, 5.0)]], KT),
    ]


def energy_chain(L=64):
    """one row per step, each with one more nested pair; energies 0, +d, 0, +d', 0 ...: consecutive differences are exactly
    +d and -d for every d of ENERGY_STEPS (0 first: two rows at the same energy)"""
    energies = [0.0]
    for d in ENERGY_STEPS:
        energies += [d, 0.0] if d else [0.0]
    return [[Row(_nested(L, k), e)] for k, e in enumerate(energies)]


def energy_graphs():
    return [(f"kt{kt}", energy_chain(), kt) for kt in ENERGY_KTS]


def star_graph(S, leaf_energy=-1.5):
    """the unfolded row as the hub and S - 1 one-pair leaves (2k, 2k+1), all at one energy"""
    L = max(2, 2 * (S - 1))
    steps = [[Row("." * L, 0.0)]]
    if S > 1:
        steps.append([Row(db_of(L, [(2 * k, 2 * k + 1)]), leaf_energy) for k in range(S - 1)])
    return steps


def star_graphs():
    return [(f"S{S}", star_graph(S), KT) for S in STAR_SIZES]


def two_state_graph(energy=-1.0, L=8):
    return [[Row("." * L, 0.0)], [Row(_nested(L, 1), energy)]]


def malformed_graphs():
    """a valid graph with one byte of its first or of its last row replaced, at position 0 or L - 1"""
    L = 66
    good = length_edge_graph(L)
    assert good[-1][-1].str_struct[0] == "." and good[-1][-1].str_struct[-1] == "."
    out = []
    for kind, ch in (("unbalanced_open", "("), ("leading_close", ")"), ("foreign_byte", "x")):
        for which in ("first", "last"):
            for pos in (0, L - 1):
                g = [[Row(r.str_struct, r.energy) for r in step] for step in good]
                row = g[0][0] if which == "first" else g[-1][-1]
                row.str_struct = row.str_struct[:pos] + ch + row.str_struct[pos + 1:]
                try:
                    parse_pairs(row.str_struct)
                except ValueError:
                    out.append((f"{kind}_{which}_row_pos{pos}", g))
                else:
                    raise AssertionError("the row is still well-formed")
    return out


FAMILIES = {
    "length_edges": length_edge_graphs,
    "step_shapes": step_shape_graphs,
    "duplicates": duplicate_graphs,
    "energies": energy_graphs,
    "stars": star_graphs,
}


def well_formed_cases():
    """[(family/name, graph, kt)] of every well-formed graph"""
    return [(f"{fam}/{name}", g, kt) for fam, make in FAMILIES.items() for name, g, kt in make()]


# ---------------------------------------------------------------- closed forms for the master-equation solvers

SOLVER_LOG_STEP = 0.35625      # the integrator takes ceil(substeps * 0.35625 / 0.3) steps per interval: 5 at substeps 4, 10 at 8
SOLVER_STAR_LEAVES = 256       # S = 257
SOLVER_STAR_ENERGY = -3.05     # 5 kT below the hub at kt 0.61: inside the 10 kT asked for the spectral case


def solver_times(first_log, n=34):
    return np.exp(first_log + SOLVER_LOG_STEP * np.arange(n))


def two_state_populations(energy, kt, times):
    """[[unfolded], [one row at `energy` < 0]] from p = (1, 0): p1(t) = k01 / (k01 + k10) * (1 - exp(-(k01 + k10) t))"""
    k01, k10 = metropolis(-energy / kt), metropolis(energy / kt)
    with mpmath.workdps(60):
        p1 = [float(mpmath.mpf(k01) / (mpmath.mpf(k01) + k10) * (1 - mpmath.exp(-(mpmath.mpf(k01) + k10) * mpmath.mpf(float(t))))) for t in times]
        p0 = [float(1 - mpmath.mpf(k01) / (mpmath.mpf(k01) + k10) * (1 - mpmath.exp(-(mpmath.mpf(k01) + k10) * mpmath.mpf(float(t))))) for t in times]
    return np.stack([np.array(p0), np.array(p1)], axis=1)


def star_populations(n_leaves, leaf_energy, kt, times):
    """hub + N leaves of one energy below it, from the hub: p0(t) = r / (N + r) + N / (N + r) * exp(-(N + r) t) with r the
    back rate, every leaf (1 - p0) / N"""
    r = mpmath.mpf(metropolis(leaf_energy / kt))
    N = mpmath.mpf(n_leaves)
    out = np.empty((len(times), n_leaves + 1))
    with mpmath.workdps(60):
        for k, t in enumerate(times):
            p0 = r / (N + r) + N / (N + r) * mpmath.exp(-(N + r) * mpmath.mpf(float(t)))
            out[k, 0] = float(p0)
            out[k, 1:] = float((1 - p0) / N)
    return out


def solver_cases():
    """name -> (graph, kt, sample times, exact populations, spectral in its valid range)"""
    t2, ts = solver_times(-4.0), solver_times(-9.0)
    cases = {"two_state": (two_state_graph(-1.0), KT, t2, two_state_populations(-1.0, KT, t2), True),
             "two_state_kt0.2": (two_state_graph(-1.0), 0.2, t2, two_state_populations(-1.0, 0.2, t2), True),
             "two_state_kt5": (two_state_graph(-1.0), 5.0, t2, two_state_populations(-1.0, 5.0, t2), True),
             "star": (star_graph(SOLVER_STAR_LEAVES + 1, SOLVER_STAR_ENERGY), KT, ts,
                      star_populations(SOLVER_STAR_LEAVES, SOLVER_STAR_ENERGY, KT, ts), True),
             # a 460 kcal drop: the back rate underflows to 0, the folded row is absorbing; 754 kT of span
             "underflow": (two_state_graph(-460.0), KT, t2, two_state_populations(-460.0, KT, t2), False)}
    return cases


def spectral_bound(energies, kt):
    """The documented error of the spectral formula is sqrt(pi_max / pi_min) * 1e-16: p = D^1/2 Q exp(Lambda t) Q^T D^-1/2 p0
    scales the start vector by up to 1 / sqrt(pi_min) and the result by up to sqrt(pi_max), so one rounding of a unit-sized
    intermediate comes out as that much in a population.  A population is a sum over S eigenmodes whose errors add at
    worst linearly: S times the figure.  The factor 100 is for the constants that bound leaves out: the backward error of
    a symmetric eigensolver is a modest multiple of the unit round-off (not one), the matrix-vector products add a few
    more, u is 1.1e-16 rather than 1e-16."""
    e = np.asarray(energies, dtype=np.float64)
    return len(e) * math.sqrt(math.exp((e.max() - e.min()) / kt)) * 1e-16 * 100
