"""The CTC prefix beam search with hotwords (csrc/ctc_beam.hip, include/pfhip_ops.h pfhip_op_ctc_prefix_beam) and its context graph
(csrc/ctx_graph.cpp, include/pfhip.h pfhip_ctx_graph_create) restated in plain Python, written from the algorithm: the search is
CtcPrefixDecoder::CtcSearch (onnxruntime/src/ctc-prefix-decoder.cpp:157-263) without its Viterbi half, the graph is what
BuildContextGraph + GetNextState (context_graph.cpp:33-118) walk.  `ft` is the number type every operation is rounded to:
np.float64 (the reference of the GPU tests) or np.float32 (the same formulas; its distance from float64 is the tests' error unit).

Order among equal totals (the reference leaves it open): unchanged hypotheses first, in beam order, then extensions,
hypothesis-major and candidate-minor; an extension that names a live hypothesis is that hypothesis."""
import numpy as np

FMAX = float(np.finfo(np.float32).max)


# ---- the context graph ------------------------------------------------------------------------------------------------------------
class Graph:
    """CSR arrays as pfhip_ctx_graph_dump returns them: arc_begin [S + 1], arc_label / arc_next / arc_weight [A], escape [S]."""

    def __init__(self, words, weights, vocab):
        f = np.float32
        inf = f(np.inf)
        nodes = [dict(child={}, end={}, min_cum=f(0), final=False, end_cum=inf)]
        for w, ws in zip(words, weights):
            assert len(w) >= 1 and len(w) == len(ws) and all(1 <= t < vocab for t in w) and np.isfinite(np.asarray(ws, f)).all()
            cum, node = f(0), 0
            for i, (t, x) in enumerate(zip(w, ws)):
                cum = f(cum + f(x))
                if i + 1 < len(w):
                    c = nodes[node]["child"].get(t)
                    if c is None:
                        c = len(nodes)
                        nodes[node]["child"][t] = c
                        nodes.append(dict(child={}, end={}, min_cum=inf, final=False, end_cum=inf))
                    nodes[c]["min_cum"] = min(nodes[c]["min_cum"], cum)
                    node = c
                else:
                    e = nodes[node]["end"]
                    e[t] = min(e[t], cum) if t in e else cum
        for u in nodes:
            for t, cum in u["end"].items():
                if t in u["child"]:
                    v = nodes[u["child"][t]]
                    v["final"] = True
                    v["end_cum"] = min(v["end_cum"], cum)
                    v["min_cum"] = min(v["min_cum"], cum)
        arcs = []
        for u in nodes:
            a = [(t, c, f(nodes[c]["min_cum"] - u["min_cum"])) for t, c in u["child"].items()]
            a += [(t, 0, f(cum - u["min_cum"])) for t, cum in u["end"].items() if t not in u["child"]]
            arcs.append(a)
        root = list(arcs[0])
        for i, u in enumerate(nodes):
            if i and u["final"]:
                r0 = f(u["end_cum"] - u["min_cum"])
                arcs[i] += [(t, n, f(r0 + w)) for t, n, w in root if t not in u["child"] and t not in u["end"]]
        self.vocab = vocab
        self.arc_begin = np.zeros(len(nodes) + 1, np.int32)
        lab, nxt, wgt = [], [], []
        for i, a in enumerate(arcs):
            for t, n, w in sorted(a, key=lambda x: x[0]):
                lab.append(t); nxt.append(n); wgt.append(w)
            self.arc_begin[i + 1] = len(lab)
        self.arc_label = np.asarray(lab, np.int32)
        self.arc_next = np.asarray(nxt, np.int32)
        self.arc_weight = np.asarray(wgt, np.float32)
        self.escape = np.asarray([f(0)] + [f(-u["min_cum"]) for u in nodes[1:]], np.float32)

    def step(self, state, tok):
        """(next state, score) of GetNextState: the arc with the label, else the escape weight and state 0."""
        lo, hi = int(self.arc_begin[state]), int(self.arc_begin[state + 1])
        i = lo + int(np.searchsorted(self.arc_label[lo:hi], tok))
        if i < hi and self.arc_label[i] == tok:
            return int(self.arc_next[i]), float(self.arc_weight[i])
        return 0, float(self.escape[state])


# ---- the search -------------------------------------------------------------------------------------------------------------------
def log_add(x, y, ft):
    if x <= -FMAX:
        return y
    if y <= -FMAX:
        return x
    m = max(x, y)
    return ft(ft(np.log(ft(ft(np.exp(ft(x - m))) + ft(np.exp(ft(y - m)))))) + m)


class _Hyp:
    __slots__ = ("prefix", "s", "ns", "ctx", "state", "slot")

    def __init__(self, prefix, s, ns, ctx, state, slot=None):
        self.prefix, self.s, self.ns, self.ctx, self.state, self.slot = prefix, s, ns, ctx, state, slot


def search(ids, logp, blank, first_beam, second_beam, graph=None, ft=np.float64, vocab=None, nbest=None):
    """ids / logp [T][k] (k >= first_beam; the first first_beam columns of a row are its candidates).  Returns a dict: hyps = a list
    of (tokens, score, ctc_score, ctx_score) in final order, prune_margin = the least (last kept - first dropped) total over the
    frames, final_margin = the least gap between neighbours of the final order up to the one behind nbest."""
    ids = np.asarray(ids)
    logp = np.asarray(logp)
    T = ids.shape[0]
    if T == 0:
        return dict(hyps=[], prune_margin=np.inf, final_margin=np.inf)
    V = vocab if vocab is not None else (graph.vocab if graph is not None else int(ids.max()) + 1)
    total = lambda h: ft(log_add(h.s, h.ns, ft) + h.ctx)
    beam = [_Hyp((), ft(0), ft(-FMAX), ft(0), 0)]
    prune_margin = np.inf
    for t in range(T):
        live = {h.prefix: i for i, h in enumerate(beam)}
        cand = {}

        def entry(prefix, slot, ctx, state):
            e = cand.get(prefix)
            if e is None:
                e = cand[prefix] = _Hyp(prefix, ft(-FMAX), ft(-FMAX), ctx, state, slot)
            return e

        for h, H in enumerate(beam):
            for c in range(first_beam):
                tok = min(max(int(ids[t, c]), 0), V - 1)
                p = ft(logp[t, c])
                if not p >= -FMAX:                                   # NaN and -inf count as "never"
                    p = ft(-FMAX)
                p = min(p, ft(FMAX))
                if tok == blank:
                    e = entry(H.prefix, (0, h, 0), H.ctx, H.state)
                    e.s = log_add(e.s, ft(log_add(H.s, H.ns, ft) + p), ft)
                    continue
                if H.prefix and tok == H.prefix[-1]:
                    e = entry(H.prefix, (0, h, 0), H.ctx, H.state)
                    e.ns = log_add(e.ns, ft(H.ns + p), ft)
                    base = H.s
                else:
                    base = log_add(H.s, H.ns, ft)
                new = H.prefix + (tok,)
                if new in live:
                    L = beam[live[new]]
                    e = entry(new, (0, live[new], 0), L.ctx, L.state)
                elif new in cand:
                    e = cand[new]
                else:
                    state, ctx = H.state, H.ctx
                    if graph is not None:
                        state, w = graph.step(H.state, tok)
                        ctx = ft(H.ctx + ft(w))
                    e = entry(new, (1, h, c), ctx, state)
                e.ns = log_add(e.ns, ft(base + p), ft)
        order = sorted(cand.values(), key=lambda e: (-_key(total(e)), e.slot))
        if len(order) > second_beam:
            prune_margin = min(prune_margin, float(total(order[second_beam - 1])) - float(total(order[second_beam])))
        beam = order[:second_beam]
    if graph is not None:
        for h in beam:
            if h.state != 0:
                h.ctx = ft(h.ctx + ft(graph.escape[h.state]))
                h.state = 0
    for i, h in enumerate(beam):
        h.slot = i
    beam.sort(key=lambda e: (-_key(total(e)), e.slot))
    n = len(beam) if nbest is None else min(nbest + 1, len(beam))
    gaps = [float(total(beam[i])) - float(total(beam[i + 1])) for i in range(n - 1)]
    hyps = [(list(h.prefix), float(total(h)), float(log_add(h.s, h.ns, ft)), float(h.ctx)) for h in beam]
    return dict(hyps=hyps if nbest is None else hyps[:nbest], prune_margin=prune_margin, final_margin=min(gaps) if gaps else np.inf)


def _key(x):
    x = float(x)
    return -np.inf if x != x else x                                  # a NaN total sorts last


def collapse(frame_ids, blank=0):
    out, prev = [], -1
    for t in frame_ids:
        if t != blank and t != prev:
            out.append(int(t))
        prev = t
    return out


def all_alignments(logp_full, blank=0):
    """{token tuple: probability} summed over every alignment of logp_full [T][V] (brute force, V ** T paths)."""
    import itertools
    T, V = logp_full.shape
    out = {}
    for path in itertools.product(range(V), repeat=T):
        p = float(np.exp(sum(float(logp_full[t, c]) for t, c in enumerate(path))))
        key = tuple(collapse(path, blank))
        out[key] = out.get(key, 0.0) + p
    return out
