"""The CTC forced alignment of csrc/ctc_align.hip restated in numpy float32 (include/pfhip_ops.h, pfhip_op_ctc_align, states it in
words), and a brute-force enumeration of all paths for small cases.  The GPU tests compare with viterbi() bit for bit.

E [N, L + 1]: column 0 the blank, column j label j (1-based).  States s = 0 .. 2 L: even = blank, odd = label (s + 1) / 2."""
import itertools

import numpy as np

NEG = np.float32(-np.inf)


def col(s):
    return (s + 1) // 2 if s & 1 else 0


def repeats(labels):
    return sum(1 for a, b in zip(labels[:-1], labels[1:]) if a == b)


def feasible(N, labels):
    """N frames can spell the labels: one frame each and a blank between equal neighbours."""
    return N >= len(labels) + repeats(labels)


def viterbi(E, labels, dtype=np.float32):
    """(score, begin [L], end [L], logp [L], path [N] of states or None).  Infeasible (score -inf): spans -1.  dtype float32 is the
    kernel's arithmetic (the bit-for-bit comparisons); float64 gives the optimum on float64 emissions."""
    F = dtype
    E = np.asarray(E, F)
    labels = [int(x) for x in labels]
    L = len(labels)
    N = E.shape[0]
    begin, end = np.full(L, -1, np.int32), np.full(L, -1, np.int32)
    logp = np.full(L, NEG, F)
    if N == 0:
        return (F(0.0) if L == 0 else F(NEG)), begin, end, logp, None
    S = 2 * L + 1
    v = np.full(S, NEG, F)
    v[0] = E[0, 0]
    if L >= 1:
        v[1] = E[0, 1]
    bp = np.zeros((N, S), np.int8)
    for t in range(1, N):
        nv = np.empty(S, F)
        for s in range(S):
            best, step = v[s], 0
            if s >= 1 and v[s - 1] > best:
                best, step = v[s - 1], 1
            if (s & 1) and s >= 3 and labels[(s + 1) // 2 - 1] != labels[(s - 1) // 2 - 1] and v[s - 2] > best:
                best, step = v[s - 2], 2
            nv[s] = F(best) + E[t, col(s)]                   # one add in the working precision
            bp[t, s] = step
        v = nv
    s = 0
    if L > 0:
        s = 2 * L if v[2 * L] >= v[2 * L - 1] else 2 * L - 1
    score = F(v[s])
    if not score > NEG:
        return F(NEG), begin, end, logp, None
    path = np.zeros(N, np.int32)
    for t in range(N - 1, -1, -1):
        path[t] = s
        if t > 0:
            s -= int(bp[t, s])
    for j in range(L):
        on = np.nonzero(path == 2 * j + 1)[0]
        begin[j], end[j] = on[0], on[-1] + 1
        logp[j] = E[on[0], j + 1]
    return score, begin, end, logp, path


def path_score(E, path):
    """The float64 sum of a path's emissions (how a path found under one E is scored on another)."""
    E = np.asarray(E, np.float64)
    return float(sum(E[t, col(int(s))] for t, s in enumerate(path)))


def path_from_spans(N, begin, end):
    """The state sequence of given spans: label j's state on [begin[j], end[j]), the blank state before / between / after."""
    path = np.zeros(N, np.int32)
    t = 0
    for j in range(len(begin)):
        path[t:begin[j]] = 2 * j
        path[begin[j]:end[j]] = 2 * j + 1
        t = end[j]
    path[t:] = 2 * len(begin)
    return path


def collapse(path, labels):
    """The labels a state path spells (CTC collapse: runs merged, blanks dropped)."""
    out, prev = [], -1
    for s in path:
        s = int(s)
        if s != prev and (s & 1):
            out.append(labels[s // 2])
        prev = s
    return out


def valid_paths(N, labels):
    """Every state sequence of length N through the trellis (brute force: N <= 5, L <= 3)."""
    L = len(labels)
    S = 2 * L + 1
    for p in itertools.product(range(S), repeat=N):
        if p[0] > 1 or p[-1] < S - 2:
            continue
        ok = True
        for a, b in zip(p[:-1], p[1:]):
            d = b - a
            if d < 0 or d > 2:
                ok = False
            elif d == 2 and not ((b & 1) and labels[(b + 1) // 2 - 1] != labels[(b - 1) // 2 - 1]):
                ok = False
            if not ok:
                break
        if ok:
            yield p


def brute_force(E, labels):
    """(best float64 score over all paths or -inf, the paths attaining it)."""
    E = np.asarray(E, np.float64)
    best, arg = -np.inf, []
    for p in valid_paths(E.shape[0], labels):
        sc = sum(E[t, col(s)] for t, s in enumerate(p))
        if sc > best:
            best, arg = sc, [p]
        elif sc == best and sc > -np.inf:
            arg.append(p)
    return best, arg
