"""CPU: the restatement tests/lm_ref.py held to brute force.  The automaton's lm_step chains against a dictionary scorer that knows
nothing of states; the search over a non-autoregressive head's candidates with the model against every sequence scored on its own; the
CTC prefix beam search with the model against the enumeration of all alignments."""
import itertools

import numpy as np
import pytest

import ctc_beam_ref as C
import lm_ref as R

F = np.float32


def dict_logprob(table, order, history, w, oov):
    """Natural-log p(w | history) by the ARPA rule, straight from the dictionary {labels: (log10 p, log10 backoff)}: the longest
    listed n-gram (context, w), every listed context dropped on the way paying its back-off; a word without a unigram scores `oov`
    behind the back-offs.  Returns (value, sum of |terms|, whether the word had a unigram)."""
    ctx = tuple(history)[-(order - 1):] if order > 1 else ()
    acc, mag = 0.0, 0.0
    while True:
        if ctx + (w,) in table:
            p = table[ctx + (w,)][0] * R.LN10
            return acc + p, mag + abs(p), True
        if not ctx:
            return acc + oov, mag + abs(oov), False
        if ctx in table:
            b = table[ctx][1] * R.LN10
            acc, mag = acc + b, mag + abs(b)
        ctx = ctx[1:]


@pytest.mark.parametrize("seed,order", [(0, 1), (1, 2), (2, 3), (3, 4), (4, 4)])
def test_step_chains_agree_with_a_dictionary_scorer(seed, order):
    """Every sequence up to length 4 over 5 tokens, from <s>, with </s> at its end: the chain of lm_step weights equals the
    dictionary's value within the float32 rounding of the baked weights (2^-24 of every term's magnitude)."""
    V = 5
    rng = np.random.default_rng(seed)
    grams = R.random_ngrams(rng, V, order, [14, 30, 40][:order - 1], missing=(3,) if seed == 4 else (), with_unk=seed == 3)
    table = {tuple(g): (p, b) for g, p, b in grams}
    lm = R.Lm(grams, V, oov_log10=-9.0)
    unk = table.get((V + 2,), (-9.0, 0.0))[0] * R.LN10
    n = 0
    for L in range(0, 5):
        for seq in itertools.product(range(V), repeat=L):
            state, hist = lm.start, (V + 1,)
            for w in seq + (V,):
                state, got = R.step(lm, state, w, np.float64)
                want, mag, listed = dict_logprob(table, order, hist, w, unk)
                assert listed or state == 0
                assert abs(float(got) - want) <= mag * 2.0 ** -23 + 1e-12, (seq, w, got, want)
                hist = hist + (w,)
                n += 1
    assert n == sum((L + 1) * V ** L for L in range(5))


def test_sentence_scorer_is_the_chain_of_steps():
    rng = np.random.default_rng(5)
    grams = R.random_ngrams(rng, 6, 3, [20, 30])
    lm = R.Lm(grams, 6, scale=0.5, token_bonus=0.25)
    tok_w, e, total = R.score_sentence(lm, [1, 2, 9, -3, 0], max_len=7)        # 9 and -3 are clamped to 5 and 0
    state, acc = lm.start, F(0)
    for i, t in enumerate([1, 2, 5, 0, 0]):
        state, w = R.step(lm, state, t)
        assert tok_w[i] == w
        acc = F(acc + w)
    assert tok_w[5] == 0 and tok_w[6] == 0 and e == R.step(lm, state, 6)[1] and total == F(acc + e)


@pytest.mark.parametrize("seed", range(4))
def test_nar_search_with_a_full_beam_is_the_exhaustive_top_n(seed):
    """Width 2, T = 4, beam 16 = 2 ** 4: nothing is ever pruned, so the search returns the best of all 16 sequences, each with the
    bits of its own left-to-right sums."""
    rng = np.random.default_rng(20 + seed)
    V, T = 8, 4
    ids = np.stack([rng.permutation(V)[:2] for _ in range(T)]).astype(np.int32)
    lp = -np.cumsum(rng.uniform(0.05, 0.6, size=(T, 2)), axis=1).astype(np.float32)
    lm = R.Lm(R.random_ngrams(rng, V, 3, [30, 40], with_eos=seed % 2 == 0), V, scale=0.8, token_bonus=0.1)
    got = R.nar_search(ids, lp, 2, 16, 16, lm, vocab=V)
    want = R.nar_brute_force(ids, lp, 2, 16, lm, vocab=V)
    assert len(got) == 16 and len({float(h[1]) for h in want}) == 16               # distinct totals: no tie rule is needed
    for g, w in zip(got, want):
        assert g[0] == w[0] and all(F(a).tobytes() == F(b).tobytes() for a, b in zip(g[1:], w[1:]))
    # and a narrow beam returns a subset in the same order
    few = R.nar_search(ids, lp, 2, 3, 2, lm, vocab=V)
    assert len(few) == 2 and few[0][0] == want[0][0]


def test_nar_search_without_weight_is_the_plain_search():
    import nar_beam_ref as N
    rng = np.random.default_rng(3)
    ids, lp = N._rows("random", 9, 1)
    lm = R.Lm(R.random_ngrams(rng, N.V, 2, [50]), N.V, scale=0.0, token_bonus=0.0)
    got = R.nar_search(ids, lp, 4, 8, 8, lm)
    want = N.search(ids, lp, 4, 8, 8)
    assert [(g[0], g[1], g[2], g[3]) for g in got] == [tuple(w) for w in want] and all(g[4] == 0 for g in got)


@pytest.mark.parametrize("T,V,seed", [(1, 2, 0), (2, 3, 1), (3, 3, 2), (4, 3, 3), (4, 2, 4)])
def test_unpruned_ctc_search_with_the_model_against_all_alignments(T, V, seed):
    """Beams wide enough that nothing is pruned: every reachable prefix's ctc score is the log of the sum over its alignments (as
    without a model), its lm score is the sentence scorer's total of that prefix, and the order is by their sum."""
    rng = np.random.default_rng(seed)
    logp = np.log(rng.dirichlet(np.ones(V), size=T))
    ids = np.tile(np.arange(V), (T, 1))
    lm = R.Lm(R.random_ngrams(rng, V, 3, [6, 8]), V, scale=0.7, token_bonus=0.2)
    paths = C.all_alignments(logp)
    r = R.ctc_search(ids, logp, 0, V, 10 ** 6, lm, ft=np.float64, vocab=V)
    assert r["prune_margin"] == np.inf
    real = [h for h in r["hyps"] if h[2] > -C.FMAX]
    assert {tuple(h[0]) for h in real} == set(paths)
    want = []
    for h in real:
        key = tuple(h[0])
        state, l = lm.start, 0.0
        for w in key + (V,):
            state, x = R.step(lm, state, w, np.float64)
            l += float(x)
        assert np.isclose(h[2], np.log(paths[key]), atol=1e-10) and np.isclose(h[4], l, atol=1e-10) and h[3] == 0
        assert np.isclose(h[1], np.log(paths[key]) + l, atol=1e-10)
        want.append((np.log(paths[key]) + l, key))
    assert [tuple(h[0]) for h in real] == [k for _, k in sorted(want, key=lambda e: -e[0])]


def test_ctc_search_with_a_weightless_model_is_the_plain_search():
    rng = np.random.default_rng(9)
    V, T = 6, 12
    logp = np.log(rng.dirichlet(np.ones(V) * 0.5, size=T))
    ids = np.argsort(-logp, axis=1, kind="stable")[:, :4]
    lp = np.take_along_axis(logp, ids, axis=1)
    lm = R.Lm(R.random_ngrams(rng, V, 2, [10]), V, scale=0.0)
    for ft in (np.float64, np.float32):
        got = R.ctc_search(ids, lp, 0, 4, 5, lm, ft=ft, vocab=V)
        want = C.search(ids, lp, 0, 4, 5, ft=ft, vocab=V)
        assert [h[:4] for h in got["hyps"]] == [tuple(h) for h in want["hyps"]] and got["prune_margin"] == want["prune_margin"]
