"""The hotword-biased beam search over a non-autoregressive head's candidates (csrc/nar_beam.hip, include/pfhip_ops.h
pfhip_op_nbest_ctx_beam) restated in numpy with np.float32 scalars: every sum is one float32 add in the order the header states, so
the device's scores are expected BIT FOR BIT.  The graph is walked from the CSR arrays pfhip_ctx_graph_dump returns (a dict, or any
object with those five attributes such as ctc_beam_ref.Graph).

Order among equal totals: hypothesis-major, candidate-minor; at the end, beam order.

`defect` seeds a mistake for tests/test_nar_beam_ref.py, which shows that the GPU test's comparison (`mismatches`) catches it on the
GPU test's own cases (`op_cases`): 1 = equal totals ordered the other way round, 2 = the escape weight of an unfinished match forgotten
at the end, 3 = candidates ordered candidate-major."""
import itertools

import numpy as np

F = np.float32
FMAX = F(np.finfo(np.float32).max)
V, K = 64, 8                                     # the operator test's vocabulary and row width


# ---- the graph ----------------------------------------------------------------------------------------------------------------------
def _arr(graph, name):
    return graph[name] if isinstance(graph, dict) else getattr(graph, name)


def step(graph, state, tok):
    """(next state, weight) of GetNextState: the arc with the label, else the state's escape weight and state 0."""
    begin, label = _arr(graph, "arc_begin"), _arr(graph, "arc_label")
    lo, hi = int(begin[state]), int(begin[state + 1])
    i = lo + int(np.searchsorted(label[lo:hi], tok))
    if i < hi and int(label[i]) == tok:
        return int(_arr(graph, "arc_next")[i]), F(_arr(graph, "arc_weight")[i])
    return 0, F(_arr(graph, "escape")[state])


def _clean(ids_row, logp_row, width, vocab):
    toks = [min(max(int(x), 0), vocab - 1) for x in ids_row[:width]]
    ps = []
    for p in logp_row[:width]:
        p = F(p)
        if not p >= -FMAX:                       # NaN and -inf count as -FLT_MAX
            p = -FMAX
        ps.append(min(p, FMAX))
    return toks, ps


def _total(am, ctx):
    with np.errstate(over="ignore", invalid="ignore"):
        t = F(am + ctx)
    return F(-np.inf) if t != t else t


# ---- the search ---------------------------------------------------------------------------------------------------------------------
def search(ids, logp, width, beam, nbest, graph=None, vocab=V, defect=0):
    """ids / logp [T][k >= width].  Returns the hypotheses in final order, at most nbest: [(tokens, score, am, ctx)], float32."""
    ids, logp = np.asarray(ids), np.asarray(logp)
    T = ids.shape[0]
    if T == 0:
        return []
    hyps = [(F(0), F(0), 0, ())]                 # am, ctx, state, tokens
    for t in range(T):
        toks, ps = _clean(ids[t], logp[t], width, vocab)
        cands = []
        for h, (am, ctx, state, seq) in enumerate(hyps):
            for c in range(width):
                with np.errstate(over="ignore"):
                    am2 = F(am + ps[c])
                state2, ctx2 = state, ctx
                if graph is not None:
                    state2, w = step(graph, state, toks[c])
                    with np.errstate(over="ignore", invalid="ignore"):
                        ctx2 = F(ctx + w)
                slot = c * len(hyps) + h if defect == 3 else h * width + c
                cands.append((_total(am2, ctx2), slot, am2, ctx2, state2, seq + (toks[c],)))
        cands.sort(key=lambda e: (-float(e[0]), -e[1] if defect == 1 else e[1]))
        hyps = [e[2:] for e in cands[:beam]]
    fin = []
    for i, (am, ctx, state, seq) in enumerate(hyps):
        if graph is not None and state != 0 and defect != 2:
            with np.errstate(over="ignore", invalid="ignore"):
                ctx = F(ctx + F(_arr(graph, "escape")[state]))
        fin.append((_total(am, ctx), i, am, ctx, seq))
    fin.sort(key=lambda e: (-float(e[0]), -e[1] if defect == 1 else e[1]))
    return [(list(seq), tot, am, ctx) for tot, _, am, ctx, seq in fin[:nbest]]


def brute_force(ids, logp, width, nbest, graph=None, vocab=V):
    """Every one of the width ** T sequences scored on its own (the same adds in the same order along the sequence, so the same
    bits), then sorted by total.  It knows no tie rule: the caller checks that the totals it compares are distinct."""
    ids, logp = np.asarray(ids), np.asarray(logp)
    T = ids.shape[0]
    rows = [_clean(ids[t], logp[t], width, vocab) for t in range(T)]
    out = []
    for choice in itertools.product(range(width), repeat=T):
        am, ctx, state = F(0), F(0), 0
        for t, c in enumerate(choice):
            am = F(am + rows[t][1][c])
            if graph is not None:
                state, w = step(graph, state, rows[t][0][c])
                ctx = F(ctx + w)
        if graph is not None and state != 0:
            ctx = F(ctx + F(_arr(graph, "escape")[state]))
        out.append((_total(am, ctx), am, ctx, [rows[t][0][c] for t, c in enumerate(choice)]))
    out.sort(key=lambda e: -float(e[0]))
    return [(seq, tot, am, ctx) for tot, am, ctx, seq in out[:nbest]]


# ---- the comparison of the GPU tests ------------------------------------------------------------------------------------------------
def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def as_outputs(hyps, nbest_stride, max_tokens):
    """The operator's six outputs of ONE utterance from a hypothesis list: (n_hyp, ids [nbest_stride][max_tokens], n_tokens, score,
    am_score, ctx_score [nbest_stride]) with the fill behind n_hyp."""
    ids = np.full((nbest_stride, max_tokens), -1, np.int32)
    n_tok = np.zeros(nbest_stride, np.int32)
    score, am = np.full(nbest_stride, -np.inf, np.float32), np.full(nbest_stride, -np.inf, np.float32)
    ctx = np.zeros(nbest_stride, np.float32)
    for j, (seq, s, a, c) in enumerate(hyps):
        n = min(len(seq), max_tokens)
        ids[j, :n] = seq[:n]
        n_tok[j] = len(seq)
        score[j], am[j], ctx[j] = s, a, c
    return np.int32(len(hyps)), ids, n_tok, score, am, ctx


def mismatches(got, want):
    """The names of the outputs of one utterance that differ: integers by value, scores by their bits.  Empty: equal."""
    names = ("n_hyp", "ids", "n_tokens", "score", "am_score", "ctx_score")
    bad = []
    for name, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        same = g.shape == w.shape and (np.array_equal(bits(g), bits(w)) if w.dtype == np.float32 else np.array_equal(g, w))
        if not same:
            bad.append(name)
    return bad


# ---- the operator test's cases ------------------------------------------------------------------------------------------------------
LENS = (0, 1, 7, 13)
DESC = ((1, 1, 1), (3, 4, 2), (8, 16, 16), (8, 16, 3))                # (width, beam, nbest) of the four utterances


def _rows(kind, T, seed):
    """T rows of K distinct ids and descending log-probabilities.  random: gaps below a hotword's weight; ties: dyadic values, the
    same in every row, so that many totals are EXACTLY equal in float32; dirty: random with a NaN, a -inf and ids out of range."""
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.permutation(np.arange(1, V))[:K] for _ in range(T)]).astype(np.int32) if T else np.zeros((0, K), np.int32)
    if kind == "ties":
        lp = np.tile(-np.arange(1, K + 1, dtype=np.float32) / 4, (T, 1))
    else:
        lp = -np.cumsum(rng.uniform(0.05, 0.6, size=(T, K)), axis=1).astype(np.float32)
    if kind == "dirty" and T:
        lp[T // 2, 1] = np.nan
        lp[T - 1, 0] = -np.inf
        ids[0, 0] = 1000
        ids[T // 3, 2] = -5
    return ids, lp.astype(np.float32)


def op_utterances(kind):
    return [_rows(kind, T, 40 + 7 * b) for b, T in enumerate(LENS)]


def op_words(utts):
    """(one word, five words with shared prefixes), each (words, weights), made of the utterances' own runner-up candidates so that
    they change the result: in the 13-row utterance a = row 3's second column, b = row 4's second, c = row 5's third, and in the 7-row
    one the word [x, y, z] starts on its last two rows (z never comes: the unfinished match whose weight is taken back at the end),
    while [p] ends on the single row of the one-row utterance and [.., q] on the last row of the 13-row one."""
    u1, u7, u13 = utts[1][0], utts[2][0], utts[3][0]
    a, b, c, d, e = int(u13[3, 1]), int(u13[4, 1]), int(u13[5, 2]), int(u13[4, 2]), int(u13[6, 1])
    x, y = int(u7[5, 1]), int(u7[6, 1])
    z = next(t for t in range(1, V) if t not in set(u7.ravel().tolist()))
    p, q0, q = int(u1[0, 1]), int(u13[11, 1]), int(u13[12, 1])
    one = ([[a, b, c]], [1.5])
    five = ([[a, b], [a, b, c, e], [a, d], [x, y, z], [q0, q], [p]], [1.25, 1.5, 0.75, 2.0, 1.75, 2.5])
    return one, five


GRAPH_SETS = ((-1, -1, -1, -1), (0, 0, 0, 0), (1, 1, 1, 1), (-1, 0, 1, 0))


def op_cases():
    """[(kind, utterances, graph words (one, five), graph_of)] of the operator test."""
    out = []
    for kind in ("random", "ties", "dirty"):
        utts = op_utterances(kind)
        words = op_words(op_utterances("random" if kind == "dirty" else kind))
        for graph_of in GRAPH_SETS:
            out.append((kind, utts, words, graph_of))
    return out


def op_reference(utts, graphs, graph_of, max_tokens, defect=0, desc=DESC):
    """The six outputs per utterance; graphs: CSR dumps (or twins) indexed by graph_of."""
    stride = max(d[2] for d in desc)
    out = []
    for (ids, lp), (w, bm, nb), g in zip(utts, desc, graph_of):
        hyps = search(ids, lp, w, bm, nb, graph=None if g < 0 else graphs[g], defect=defect)
        out.append(as_outputs(hyps, stride, max_tokens))
    return out
