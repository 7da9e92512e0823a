"""A numpy restatement of the maximum-expected-accuracy recursion of include/rafft_hip.h (rafft_mea_batch): from P (only [i][j],
i < j, is read), the stored unpaired probabilities q and gamma: W = (gamma + gamma) P rounded once, the table
E[i][j] = max(E[i][j-1] + q_j, max over k of (E[i][k-1] + W(k,j)) + E[k+1][j-1]) over the cells with P(k,j) > 0, and the traceback
with its fixed order.  fp64 additions in the stated association only: the bits are the device's.  Test infrastructure."""
import math

import numpy as np


def unpaired(P):
    """q from P as the definition forms it: the partners of i in ascending index, one running sum, clamped at 0"""
    L = P.shape[0]
    q = np.zeros(L)
    for i in range(L):
        s = 0.0
        for p in range(L):
            if p != i:
                s += float(P[min(p, i), max(p, i)])
        q[i] = max(0.0, 1.0 - s)
    return q


def table(P, q, gamma):
    """(E, W, cands): E is (L + 1) x (L + 1) - column L and row L stay 0, so that E[i][-1] and every E[i][j] with j < i read 0"""
    L = len(q)
    P = np.asarray(P, dtype=np.float64)
    W = np.float64(gamma + gamma) * P
    cands = [np.nonzero(P[:j, j] > 0.0)[0] for j in range(L)]
    E = np.zeros((L + 1, L + 1))
    for d in range(L):
        for i in range(L - d):
            j = i + d
            best = E[i, j - 1] + q[j]
            ks = cands[j]
            ks = ks[np.searchsorted(ks, i):]
            if ks.size:
                v = (E[i, ks - 1] + W[ks, j]) + E[ks + 1, j - 1]
                best = max(best, v.max())
            E[i, j] = best
    return E, W, cands


def traceback(E, W, cands, q, last=False, stats=None):
    """the row; last=True: the LAST reproducing candidate instead of the first - a variant the tests must tell from the definition.
    stats["rounds"]: the rounds of 64 candidates the longest search for a partner takes when the candidates are tested 64 at a time
    from the interval's first position"""
    L = len(q)
    row = ["."] * L
    stack = [(0, L - 1)]
    while stack:
        i, j = stack.pop()
        while j >= i:
            if E[i, j] == E[i, j - 1] + q[j]:
                j -= 1
                continue
            ks = cands[j]
            ks = ks[np.searchsorted(ks, i):]
            v = (E[i, ks - 1] + W[ks, j]) + E[ks + 1, j - 1]
            hits = ks[v == E[i, j]]
            if not hits.size:
                raise AssertionError(f"cell ({i},{j}) is reproduced by nothing")
            k = int(hits[-1] if last else hits[0])
            if stats is not None:
                stats["rounds"] = max(stats.get("rounds", 0), (k - i) // 64 + 1)
            row[k], row[j] = "(", ")"
            stack.append((i, k - 1))
            stack.append((k + 1, j - 1))
            break
    return "".join(row)


def mea(P, q, gamma, last=False):
    """(row, mea) of the definition"""
    q = np.asarray(q, dtype=np.float64)
    E, W, cands = table(P, q, gamma)
    return traceback(E, W, cands, q, last), float(E[0, len(q) - 1])


def pairs_of(row):
    stack, out = [], []
    for j, ch in enumerate(row):
        if ch == "(":
            stack.append(j)
        elif ch == ")":
            out.append((stack.pop(), j))
    assert not stack
    return out


def expected_accuracy(row, P, q, gamma):
    """sum of 2 gamma P over the pairs of the row and of q over its unpaired positions (fsum)"""
    pr = pairs_of(row)
    paired = {x for p in pr for x in p}
    return math.fsum([2.0 * gamma * float(P[i, j]) for i, j in pr] + [float(q[x]) for x in range(len(row)) if x not in paired])


def structures_over(P):
    """every non-crossing set of cells with P > 0 (i < j), as rows"""
    L = P.shape[0]
    memo = {}

    def rec(i, j):                  # the pair sets of positions i..j
        if j < i:
            return [()]
        if (i, j) not in memo:
            out = list(rec(i, j - 1))
            for k in range(i, j):
                if P[k, j] > 0.0:
                    inner = rec(k + 1, j - 1)
                    for a in rec(i, k - 1):
                        for b in inner:
                            out.append(a + ((k, j),) + b)
            memo[(i, j)] = out
        return memo[(i, j)]

    rows = []
    for ps in rec(0, L - 1):
        r = ["."] * L
        for i, j in ps:
            r[i], r[j] = "(", ")"
        rows.append("".join(r))
    return rows


def diversity(P):
    """sum over i < j of 2 P (1 - P) (fsum)"""
    iu = np.triu_indices(P.shape[0], 1)
    x = np.asarray(P, dtype=np.float64)[iu]
    return math.fsum((2.0 * x * (1.0 - x)).tolist())
