"""The token n-gram language model of the device searches restated in plain Python, written from include/pfhip.h: the builder of the
back-off automaton (csrc/lm_graph.cpp: same numbering, same double -> float rule, so pfhip_lm_graph_dump is expected BIT FOR BIT),
one step of it (csrc/lm_step.h), the sentence scorer (csrc/lm_score.hip) and the two searches with the model fused in
(csrc/nar_beam.hip, csrc/ctc_beam.hip; the searches without it are nar_beam_ref.py and ctc_beam_ref.py, unchanged).

Labels: 0 .. vocab - 1 token ids, vocab </s>, vocab + 1 <s>, vocab + 2 <unk>."""
import numpy as np

import ctc_beam_ref as cref
import nar_beam_ref as nref

F = np.float32
LN10 = 2.302585092994046
FMAX = cref.FMAX


def bake(log10v, scale, bonus):
    """fl32((log10 * ln10) * scale + bonus): Python floats are IEEE doubles and nothing here is fused."""
    t = float(log10v) * LN10
    t = t * float(scale)
    t = t + float(bonus)
    return F(t)


class Lm:
    """ngrams: (labels, log10_prob, log10_backoff) in any sequence.  Attributes as LmGraph.dump() names them."""

    def __init__(self, ngrams, vocab, scale=1.0, token_bonus=0.0, oov_log10=-10.0, order=None):
        V, eos, bos, unk = vocab, vocab, vocab + 1, vocab + 2
        scale, bonus, oov = float(F(scale)), float(F(token_bonus)), float(F(oov_log10))
        order = max([len(g[0]) for g in ngrams] + [1]) if order is None else order
        unk_p = None
        kept = [dict() for _ in range(order + 1)]                    # length -> {labels: (p, b)}
        for n in range(1, order + 1):
            for lab, p, b in ngrams:
                lab = tuple(int(t) for t in lab)
                if len(lab) != n:
                    continue
                assert all(0 <= t <= unk for t in lab) and (unk not in lab or n == 1)
                if lab[-1] == unk:
                    unk_p = p
                elif n > 1 and (lab[-1] == bos or lab[:-1] not in kept[n - 1]):
                    continue                                         # predicts <s>, or its history is not listed
                else:
                    assert lab not in kept[n]
                    kept[n][lab] = (p, b)
        state = {(): 0}
        for m in range(1, order):
            for lab in sorted(kept[m]):
                state[lab] = len(state)
        S = len(state)

        def state_of(seq):
            for m in range(min(len(seq), order - 1), 0, -1):
                if seq[len(seq) - m:] in state:
                    return state[seq[len(seq) - m:]]
            return 0

        self.vocab, self.order = V, order
        self.start = state.get((bos,), 0)
        self.has_eos = int((eos,) in kept[1])
        self.uni_w = np.full(V + 1, bake(oov if unk_p is None else unk_p, scale, bonus), np.float32)
        self.uni_w[V] = 0
        self.uni_next = np.zeros(V + 1, np.int32)
        for (w,), (p, _) in kept[1].items():
            if w != bos:
                self.uni_w[w] = bake(p, scale, 0.0 if w == eos else bonus)
                self.uni_next[w] = state.get((w,), 0)
        self.backoff_w = np.zeros(S, np.float32)
        self.backoff_state = np.zeros(S, np.int32)
        self.arc_begin = np.zeros(S + 1, np.int32)
        lab_, nxt_, wgt_ = [], [], []
        by_state = sorted(state.items(), key=lambda kv: kv[1])
        of_history = {}
        for n in range(2, order + 1):
            for g in kept[n]:
                of_history.setdefault(g[:-1], []).append(g)
        for h, s in by_state[1:]:
            self.backoff_w[s] = bake(kept[len(h)][h][1], scale, 0.0)
            self.backoff_state[s] = state_of(h[1:])
            assert self.backoff_state[s] < s and (self.backoff_state[s] == 0 or len(by_state[self.backoff_state[s]][0]) < len(h))
            for full in sorted(of_history.get(h, [])):
                w = full[-1]
                lab_.append(w); nxt_.append(state_of(full)); wgt_.append(bake(kept[len(full)][full][0], scale, 0.0 if w == eos else bonus))
            self.arc_begin[s + 1] = len(lab_)
        self.arc_label = np.asarray(lab_, np.int32)
        self.arc_next = np.asarray(nxt_, np.int32)
        self.arc_weight = np.asarray(wgt_, np.float32)

    def dump(self):
        names = ("uni_w", "uni_next", "arc_begin", "backoff_w", "backoff_state", "arc_label", "arc_next", "arc_weight", "start", "has_eos")
        return {k: getattr(self, k) for k in names}


ORDER_MAX = 6


def step(lm, state, label, ft=F):
    """(next state, acc) of lm_step; every add rounded to ft (the device's is float32)."""
    acc = ft(0)
    label = min(max(int(label), 0), lm.vocab)
    for _ in range(ORDER_MAX):
        if state == 0:
            break
        lo, hi = int(lm.arc_begin[state]), int(lm.arc_begin[state + 1])
        i = lo + int(np.searchsorted(lm.arc_label[lo:hi], label))
        if i < hi and int(lm.arc_label[i]) == label:
            return int(lm.arc_next[i]), ft(acc + ft(lm.arc_weight[i]))
        acc = ft(acc + ft(lm.backoff_w[state]))
        state = int(lm.backoff_state[state])
    return int(lm.uni_next[label]), ft(acc + ft(lm.uni_w[label]))


def score_sentence(lm, ids, max_len=None):
    """(tok_w [max_len], eos_w, total) of pfhip_op_lm_score for one sentence, float32."""
    max_len = len(ids) if max_len is None else max_len
    tok_w = np.zeros(max_len, np.float32)
    state, total = lm.start, F(0)
    for i, t in enumerate(ids):
        state, w = step(lm, state, min(max(int(t), 0), lm.vocab - 1))
        tok_w[i] = w
        total = F(total + w)
    e = F(0)
    if lm.has_eos:
        _, e = step(lm, state, lm.vocab)
        total = F(total + e)
    return tok_w, e, total


# ---- the search over a non-autoregressive head's candidates, with the model -----------------------------------------------------------
def _total3(am, ctx, l):
    with np.errstate(over="ignore", invalid="ignore"):
        t = F(F(am + ctx) + l)
    return F(-np.inf) if t != t else t


def nar_search(ids, logp, width, beam, nbest, lm, graph=None, vocab=nref.V):
    """nar_beam_ref.search with (lm, lm_state) per hypothesis.  Returns [(tokens, score, am, ctx, lm)] in final order, float32."""
    ids, logp = np.asarray(ids), np.asarray(logp)
    T = ids.shape[0]
    if T == 0:
        return []
    hyps = [(F(0), F(0), 0, F(0), lm.start, ())]                     # am, ctx, state, lm, lm_state, tokens
    for t in range(T):
        toks, ps = nref._clean(ids[t], logp[t], width, vocab)
        cands = []
        for h, (am, ctx, state, l, ls, seq) in enumerate(hyps):
            for c in range(width):
                with np.errstate(over="ignore", invalid="ignore"):
                    am2 = F(am + ps[c])
                    state2, ctx2 = state, ctx
                    if graph is not None:
                        state2, w = nref.step(graph, state, toks[c])
                        ctx2 = F(ctx + w)
                    ls2, lw = step(lm, ls, toks[c])
                    l2 = F(l + lw)
                cands.append((_total3(am2, ctx2, l2), h * width + c, am2, ctx2, state2, l2, ls2, seq + (toks[c],)))
        cands.sort(key=lambda e: (-float(e[0]), e[1]))
        hyps = [e[2:] for e in cands[:beam]]
    fin = []
    for i, (am, ctx, state, l, ls, seq) in enumerate(hyps):
        with np.errstate(over="ignore", invalid="ignore"):
            if graph is not None and state != 0:
                ctx = F(ctx + F(nref._arr(graph, "escape")[state]))
            if lm.has_eos:
                l = F(l + step(lm, ls, lm.vocab)[1])
        fin.append((_total3(am, ctx, l), i, am, ctx, l, seq))
    fin.sort(key=lambda e: (-float(e[0]), e[1]))
    return [(list(seq), tot, am, ctx, l) for tot, _, am, ctx, l, seq in fin[:nbest]]


def nar_brute_force(ids, logp, width, nbest, lm, vocab=nref.V):
    """Every one of the width ** T sequences scored on its own, sorted by total (no tie rule: the caller checks distinctness)."""
    import itertools
    ids, logp = np.asarray(ids), np.asarray(logp)
    T = ids.shape[0]
    rows = [nref._clean(ids[t], logp[t], width, vocab) for t in range(T)]
    out = []
    for choice in itertools.product(range(width), repeat=T):
        am, l, ls = F(0), F(0), lm.start
        for t, c in enumerate(choice):
            am = F(am + rows[t][1][c])
            ls, w = step(lm, ls, rows[t][0][c])
            l = F(l + w)
        if lm.has_eos:
            l = F(l + step(lm, ls, lm.vocab)[1])
        out.append((_total3(am, F(0), l), am, l, [rows[t][0][c] for t, c in enumerate(choice)]))
    out.sort(key=lambda e: -float(e[0]))
    return [(seq, tot, am, F(0), l) for tot, am, l, seq in out[:nbest]]


def nar_as_outputs(hyps, nbest_stride, max_tokens):
    """The operator's seven outputs of one utterance: nar_beam_ref.as_outputs and lm_score [nbest_stride] (0 behind n_hyp)."""
    six = nref.as_outputs([h[:4] for h in hyps], nbest_stride, max_tokens)
    l = np.zeros(nbest_stride, np.float32)
    for j, h in enumerate(hyps):
        l[j] = h[4]
    return six + (l,)


def nar_mismatches(got, want):
    bad = nref.mismatches(got[:6], want[:6])
    if not np.array_equal(nref.bits(got[6]), nref.bits(want[6])):
        bad.append("lm_score")
    return bad


# ---- the CTC prefix beam search, with the model --------------------------------------------------------------------------------------
class _Hyp:
    __slots__ = ("prefix", "s", "ns", "ctx", "state", "lm", "lm_state", "slot")

    def __init__(self, prefix, s, ns, ctx, state, lm, lm_state, slot=None):
        self.prefix, self.s, self.ns, self.ctx, self.state, self.lm, self.lm_state, self.slot = prefix, s, ns, ctx, state, lm, lm_state, slot


def ctc_search(ids, logp, blank, first_beam, second_beam, lm, graph=None, ft=np.float64, vocab=None, nbest=None):
    """ctc_beam_ref.search with (lm, lm_state) per hypothesis: a function of the prefix alone, so an unchanged hypothesis and a
    merged extension keep the live hypothesis's, and a new extension h + tok gets lm_h + acc(step(lm_state_h, tok)).  total =
    (log_add(s, ns) + ctx) + lm.  End, behind the context back-off: with </s> in the model, lm += acc(step(lm_state, vocab)).
    Returns ctc_beam_ref.search's dict with hyps = (tokens, score, ctc_score, ctx_score, lm_score)."""
    log_add, _key = cref.log_add, cref._key
    ids, logp = np.asarray(ids), np.asarray(logp)
    T = ids.shape[0]
    if T == 0:
        return dict(hyps=[], prune_margin=np.inf, final_margin=np.inf)
    V = vocab if vocab is not None else lm.vocab
    total = lambda h: ft(ft(log_add(h.s, h.ns, ft) + h.ctx) + h.lm)
    beam = [_Hyp((), ft(0), ft(-FMAX), ft(0), 0, ft(0), lm.start)]
    prune_margin = np.inf
    for t in range(T):
        live = {h.prefix: i for i, h in enumerate(beam)}
        cand = {}

        def entry(prefix, slot, src):
            e = cand.get(prefix)
            if e is None:
                e = cand[prefix] = _Hyp(prefix, ft(-FMAX), ft(-FMAX), src[0], src[1], src[2], src[3], slot)
            return e

        for h, H in enumerate(beam):
            own = (H.ctx, H.state, H.lm, H.lm_state)
            for c in range(first_beam):
                tok = min(max(int(ids[t, c]), 0), V - 1)
                p = ft(logp[t, c])
                if not p >= -FMAX:
                    p = ft(-FMAX)
                p = min(p, ft(FMAX))
                if tok == blank:
                    e = entry(H.prefix, (0, h, 0), own)
                    e.s = log_add(e.s, ft(log_add(H.s, H.ns, ft) + p), ft)
                    continue
                if H.prefix and tok == H.prefix[-1]:
                    e = entry(H.prefix, (0, h, 0), own)
                    e.ns = log_add(e.ns, ft(H.ns + p), ft)
                    base = H.s
                else:
                    base = log_add(H.s, H.ns, ft)
                new = H.prefix + (tok,)
                if new in live:
                    L = beam[live[new]]
                    e = entry(new, (0, live[new], 0), (L.ctx, L.state, L.lm, L.lm_state))
                elif new in cand:
                    e = cand[new]
                else:
                    state, ctx = H.state, H.ctx
                    if graph is not None:
                        state, w = graph.step(H.state, tok)
                        ctx = ft(H.ctx + ft(w))
                    ls, lw = step(lm, H.lm_state, tok, ft)
                    e = entry(new, (1, h, c), (ctx, state, ft(H.lm + lw), ls))
                e.ns = log_add(e.ns, ft(base + p), ft)
        order = sorted(cand.values(), key=lambda e: (-_key(total(e)), e.slot))
        if len(order) > second_beam:
            prune_margin = min(prune_margin, float(total(order[second_beam - 1])) - float(total(order[second_beam])))
        beam = order[:second_beam]
    for h in beam:
        if graph is not None and h.state != 0:
            h.ctx = ft(h.ctx + ft(graph.escape[h.state]))
            h.state = 0
        if lm.has_eos:
            h.lm = ft(h.lm + step(lm, h.lm_state, lm.vocab, ft)[1])
    for i, h in enumerate(beam):
        h.slot = i
    beam.sort(key=lambda e: (-_key(total(e)), e.slot))
    n = len(beam) if nbest is None else min(nbest + 1, len(beam))
    gaps = [float(total(beam[i])) - float(total(beam[i + 1])) for i in range(n - 1)]
    hyps = [(list(h.prefix), float(total(h)), float(log_add(h.s, h.ns, ft)), float(h.ctx), float(h.lm)) for h in beam]
    return dict(hyps=hyps if nbest is None else hyps[:nbest], prune_margin=prune_margin, final_margin=min(gaps) if gaps else np.inf)


# ---- n-gram sets for the tests -------------------------------------------------------------------------------------------------------
def random_ngrams(rng, vocab, order, per_order, with_bos=True, with_eos=True, with_unk=False, missing=()):
    """A random, prefix-closed n-gram set: every unigram but `missing`, then per_order[n - 2] n-grams of each longer length whose history
    is a listed (n - 1)-gram.  Probabilities in -0.1 .. -3, back-offs in -1 .. 0, rounded to 4 decimals as an ARPA file prints them."""
    eos, bos, unk = vocab, vocab + 1, vocab + 2
    r = lambda lo, hi: round(float(rng.uniform(lo, hi)), 4)
    grams = {}
    for w in range(vocab):
        if w not in missing:
            grams[(w,)] = (r(-3, -0.1), r(-1, 0))
    if with_eos:
        grams[(eos,)] = (r(-3, -0.1), 0.0)
    if with_bos:
        grams[(bos,)] = (-99.0, r(-1, 0))
    if with_unk:
        grams[(unk,)] = (r(-6, -4), 0.0)
    prev = [g for g in grams if g[0] not in (eos, unk)]
    for n in range(2, order + 1):
        cur = []
        words = [w for w in range(vocab) if w not in missing] + ([eos] if with_eos else [])
        for _ in range(per_order[n - 2] * 4):
            if len(cur) >= per_order[n - 2] or not prev:
                break
            h = prev[int(rng.integers(len(prev)))]
            g = h + (words[int(rng.integers(len(words)))],)
            if g not in grams:
                grams[g] = (r(-3, -0.1), r(-1, 0) if n < order else 0.0)
                cur.append(g)
        prev = [g for g in cur if g[-1] != eos]
    return [(g, p, b) for g, (p, b) in grams.items()]


def arpa_text(ngrams, names, vocab, order=None):
    """The n-grams as an ARPA file's text; names [vocab]: the token strings."""
    word = lambda t: names[t] if t < vocab else {vocab: "</s>", vocab + 1: "<s>", vocab + 2: "<unk>"}[t]
    order = max(len(g[0]) for g in ngrams) if order is None else order
    out = ["", "\\data\\"]
    for n in range(1, order + 1):
        out.append("ngram %d=%d" % (n, sum(1 for g in ngrams if len(g[0]) == n)))
    for n in range(1, order + 1):
        out += ["", "\\%d-grams:" % n]
        for lab, p, b in ngrams:
            if len(lab) == n:
                out.append("\t".join([repr(float(p)), " ".join(word(t) for t in lab)] + ([repr(float(b))] if n < order else [])))
    out += ["", "\\end\\", ""]
    return "\n".join(out)
