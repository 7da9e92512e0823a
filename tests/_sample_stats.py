"""The statistical check of the sampling tests (test infrastructure; no GPU, no product code): is a count X out of N draws what an
event of exact probability p gives?  No excluded cases and no tuned threshold.  With v = N p (1 - p), Bernstein's inequality bounds
P(|X - N p| >= t) by 2 exp(-t^2 / (2 (v + t / 3))); solving 2 exp(...) = 1e-9 for t, with a = ln(2e9):
    t = a / 3 + sqrt(a^2 / 9 + 2 a v)
so a correct sampler misses one comparison with probability at most 1e-9, whatever p and N, and a suite of 1e5 comparisons with at
most 1e-4.  Rows are a function of the seed: a pass is a pass for good.  p == 0 must give X == 0 (t = 2 a / 3 would allow 14)."""
import math

import numpy as np

A = math.log(2e9)


def allowed(n, p):
    """the largest |X - n p| the check lets pass (array or scalar p)"""
    p = np.asarray(p, dtype=np.float64)
    v = n * p * (1.0 - p)
    return A / 3.0 + np.sqrt(A * A / 9.0 + 2.0 * A * v)


def misses(counts, n, p):
    """indices of the comparisons that fail: counts[x] out of n draws against probability p[x]"""
    counts, p = np.asarray(counts, dtype=np.float64), np.asarray(p, dtype=np.float64)
    bad = np.abs(counts - n * p) > allowed(n, p)
    bad |= (p == 0.0) & (counts != 0)
    return np.nonzero(bad.ravel())[0]
