"""GPU: the CTC prefix beam search with a token n-gram language model fused in (csrc/ctc_beam.hip, the kLm instantiation) through
pfhip_op_ctc_prefix_beam_multi_lm on hand-made [rows][k] arrays, against the plain-Python restatement tests/lm_ref.py (which
tests/test_lm_ref.py holds to the enumeration of all alignments).

The rule is that of tests/test_gpu_ctc_prefix_beam_op.py, taken over unchanged: let e be the largest difference between the
restatement run in float32 and in float64 over the scores of the case (total, ctc, context and lm score of every returned
hypothesis).  The device's hypotheses must be the float64 restatement's, in order, with every score within 4 e.  Which hypotheses
survive is only well defined where no decision is closer than the arithmetic's error, so each case first asserts that every prune
margin (last kept - first dropped total, every frame) and every margin of the final order of the float64 run is at least 16 e; the
seeds below were chosen on the CPU, and a margin below that fails the test.  Rows and the model's baked weights are float32 values,
so both runs and the device read the same numbers.  e, the margins and the device's error are printed."""
import functools
import importlib

import numpy as np
import pytest

import ctc_beam_ref as C
import lm_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

A, B = 1, 2


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def rows_of(logp_full, k):
    logp_full = np.asarray(logp_full, np.float64)
    ids = np.argsort(-logp_full, axis=1, kind="stable")[:, :k]
    return ids.astype(np.int32), np.take_along_axis(logp_full, ids, axis=1).astype(np.float32)


def random_rows(T, V, k, seed, conc=0.3):
    rng = np.random.default_rng(seed)
    return rows_of(np.log(rng.dirichlet(np.ones(V) * conc, size=T) + 1e-12), k)


def hand(P):
    P = np.asarray(P, np.float64)
    return rows_of(P, P.shape[1])


def model(V, seed, order=3, per_order=(60, 80, 60), **kw):
    grams = R.random_ngrams(np.random.default_rng(seed), V, order, list(per_order)[:order - 1], missing=(V - 1,))
    kw = dict(dict(scale=0.3, token_bonus=0.1, oov_log10=-5.0), **kw)
    return grams, kw


class Case:
    """utts: a list of (ids [T][k], logp [T][k]); lm: (ngrams, LmGraph keywords); graph_words: (words, weights) or None."""

    def __init__(self, utts, V, fb, sb, lm, nbest=None, graph_words=None, max_tokens=None):
        self.utts, self.V, self.fb, self.sb, self.lm = utts, V, fb, sb, lm
        self.nbest = sb if nbest is None else nbest
        self.graph_words, self.max_tokens = graph_words, max_tokens

    def oracle(self, ft):
        twin = R.Lm(self.lm[0], self.V, **self.lm[1])
        g = None
        if self.graph_words is not None:
            words, per_word = self.graph_words
            g = C.Graph(words, [[w] * len(x) for x, w in zip(words, per_word)], self.V)
        return [R.ctc_search(i, l, 0, self.fb, self.sb, twin, graph=g, ft=ft, vocab=self.V, nbest=self.nbest) for i, l in self.utts]


PM = np.log(np.array([[.1, .6, .3], [.2, .15, .65], [.25, .2, .55]]))     # [a b] arrives as an extension and is live already
AA = [np.log([[.1, .8, .1], [.15, .8, .05]]), np.log([[.1, .8, .1], [.8, .15, .05], [.2, .7, .1]])]
SMALL_LM = ([((0,), -1.0, 0.0), ((A,), -0.4, -0.2), ((B,), -0.7, -0.3), ((3,), -1.3, 0.0), ((4,), -99.0, -0.1), ((4, A), -0.2, -0.1),
             ((A, B), -0.15, 0.0), ((A, A), -0.9, -0.05), ((B, 3), -0.3, 0.0), ((A, 3), -0.5, 0.0), ((4, A, A), -0.6, 0.0)],
            dict(scale=0.5, token_bonus=0.05))


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "merge":
        return Case([hand(PM)], 3, 3, 8, SMALL_LM, nbest=3)
    if name == "a_a":                            # a a -> [a]; a blank a -> [a a]
        return Case([hand(AA[0]), hand(AA[1])], 3, 3, 3, SMALL_LM)
    if name == "beam_16_16":
        return Case([random_rows(12, 24, 16, 21, conc=2.0)], 24, 16, 16, model(24, 5), nbest=4)
    if name == "packed_37_0_300":
        return Case([random_rows(37, 50, 5, 101, conc=.02), random_rows(0, 50, 5, 0), random_rows(300, 50, 5, 106, conc=.005)], 50, 5, 5,
                    model(50, 11, per_order=(400, 400), scale=0.05, token_bonus=0.02), nbest=3)
    base = random_rows(40, 50, 5, 7)
    if name == "short_ids":
        return Case([base], 50, 5, 5, model(50, 11, per_order=(400, 400), scale=0.15), nbest=2, max_tokens=3)
    plain = C.search(base[0], base[1], 0, 5, 5, vocab=50)["hyps"]
    best, second = plain[0][0], plain[1][0]
    if name == "with_hotwords":                  # the model and a graph together: a hotword of the runner-up's, one of the best's
        return Case([base], 50, 5, 5, model(50, 14, per_order=(400, 400)), nbest=3, graph_words=([second[13:16], best[1:3]], [0.75, 0.25]))
    if name == "lm_flip":                        # flat unigrams, and every bigram of the runner-up liked: it overtakes the best
        grams = [((w,), -1.7, -0.1) for w in range(50)] + [((50,), -1.7, 0.0), ((51,), -99.0, -0.1)]
        seen = set()
        for x, y in zip([51] + second, second):
            if (x, y) not in seen:
                seen.add((x, y))
                grams.append(((x, y), -0.4, -0.1))
        return Case([base], 50, 5, 5, (grams, dict(scale=1.0, token_bonus=0.0)), nbest=3)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 results per utterance, e, least prune margin, least final margin)."""
    c = case(name)
    r64, r32 = c.oracle(np.float64), c.oracle(np.float32)
    e, prune, final = 0.0, np.inf, np.inf
    for a, b in zip(r64, r32):
        assert [h[0] for h in a["hyps"]] == [h[0] for h in b["hyps"]], f"{name}: float32 and float64 disagree — choose another seed"
        for x, y in zip(a["hyps"], b["hyps"]):
            assert x[2] > -1e30, f"{name}: a hypothesis without a path is among the n best — choose other inputs"
            e = max(e, max(abs(x[i] - y[i]) for i in (1, 2, 3, 4)))
        prune, final = min(prune, a["prune_margin"]), min(final, a["final_margin"])
    return r64, e, prune, final


def tensors(c):
    k = c.utts[0][0].shape[1]
    ids = np.concatenate([u[0] for u in c.utts]).reshape(-1, k)
    lp = np.concatenate([u[1] for u in c.utts]).reshape(-1, k)
    lens = [len(u[0]) for u in c.utts]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    pad = lambda a, dt: torch.from_numpy(np.concatenate([a, np.zeros((1, k), dt)]).astype(dt)).cuda()      # never an empty tensor
    return (pad(ids, np.int32)[:len(ids)], pad(lp, np.float32)[:len(ids)], torch.from_numpy(offs).cuda(),
            torch.tensor(lens, dtype=torch.int32).cuda(), lens)


def run(ops, pkg, c, with_lm=True):
    ids, lp, off, n, lens = tensors(c)
    nu = len(lens)
    graphs = [] if c.graph_words is None else [pkg.ContextGraph(c.graph_words[0], c.graph_words[1], c.V)]
    lm = pkg.LmGraph.from_ngrams(c.lm[0], c.V, **c.lm[1]) if with_lm else None
    mt = max(lens) if c.max_tokens is None else c.max_tokens
    out = ops.ctc_prefix_beam_multi_lm(ids, lp, off, n, c.V, [c.fb] * nu, [c.sb] * nu, [c.nbest] * nu, lm, graph_of=[0 if graphs else -1] * nu,
                                       graphs=graphs, max_tokens=mt)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def check(ops, pkg, name):
    c = case(name)
    r64, e, prune, final = reference(name)
    print(f"{name}: e {e:.3e}  least prune margin {prune:.3e}  least final margin {final:.3e}")
    assert prune >= 16 * e and final >= 16 * e, f"{name}: a decision closer than 16 e — choose another seed"
    n_hyp, ids, n_tok, score, ctc, ctx, lms = run(ops, pkg, c)
    mt = ids.shape[2]
    worst = 0.0
    for b, r in enumerate(r64):
        want = r["hyps"]
        assert n_hyp[b] == len(want), (name, b, n_hyp[b], len(want))
        for j, (toks, s, cs, cx, l) in enumerate(want):
            assert n_tok[b, j] == len(toks), (name, b, j)
            assert ids[b, j, :min(len(toks), mt)].tolist() == toks[:mt], (name, b, j)
            assert (ids[b, j, len(toks):] == -1).all()
            worst = max(worst, abs(score[b, j] - s), abs(ctc[b, j] - cs), abs(ctx[b, j] - cx), abs(lms[b, j] - l))
        assert (n_tok[b, len(want):] == 0).all() and (ids[b, len(want):] == -1).all() and np.isneginf(score[b, len(want):]).all()
        assert (lms[b, len(want):] == 0).all()
    print(f"{name}: device error {worst:.3e}  bound {4 * e:.3e}")
    assert worst <= 4 * e, (name, worst, 4 * e)
    return r64, (n_hyp, ids, n_tok, score, ctc, ctx, lms)


@pytest.mark.parametrize("name", ["merge", "a_a"])
def test_hand_cases_with_a_model(ops, pkg, name):
    """An extension that names a live hypothesis is added to it and keeps that one's model state and score; a a -> [a] and a blank
    a -> [a a], whose model score counts a twice."""
    r64, (n_hyp, ids, n_tok, score, ctc, ctx, lms) = check(ops, pkg, name)
    twin = R.Lm(SMALL_LM[0], 3, **SMALL_LM[1])
    for b in range(len(r64)):
        seqs = [tuple(ids[b, j, :n_tok[b, j]]) for j in range(n_hyp[b])]
        assert len(set(seqs)) == len(seqs)
        for j, s in enumerate(seqs):                                 # the model's share is the sentence scorer's total of the prefix
            assert abs(lms[b, j] - R.score_sentence(twin, s)[2]) <= 1e-5
    if name == "a_a":
        assert [A, A] in [h[0] for h in r64[1]["hyps"]]


@pytest.mark.parametrize("name", ["beam_16_16", "packed_37_0_300"])
def test_widths_and_packing(ops, pkg, name):
    """16/16 at V = 24, T = 12: all 256 (hypothesis, candidate) pairs are live from the fourth frame on.  Three utterances of 37, 0
    and 300 rows in one launch: the rowless one has no hypothesis."""
    r64, (n_hyp, *_) = check(ops, pkg, name)
    if name == "packed_37_0_300":
        assert n_hyp.tolist() == [3, 0, 3]


def test_model_and_hotword_graph_together(ops, pkg):
    r64, (n_hyp, ids, n_tok, score, ctc, ctx, lms) = check(ops, pkg, "with_hotwords")
    assert (ctx[0, :n_hyp[0]] != 0).any() and (lms[0, :n_hyp[0]] != 0).all()


def test_the_model_flips_the_best_hypothesis(ops, pkg):
    r64, (n_hyp, ids, n_tok, score, ctc, ctx, lms) = check(ops, pkg, "lm_flip")
    c = case("lm_flip")
    plain = C.search(c.utts[0][0], c.utts[0][1], 0, 5, 5, vocab=50)["hyps"]
    assert r64[0]["hyps"][0][0] == plain[1][0] != plain[0][0]
    twin = R.Lm(c.lm[0], c.V, **c.lm[1])                             # what the model gives the runner-up over the former best
    gain = float(R.score_sentence(twin, plain[1][0])[2]) - float(R.score_sentence(twin, plain[0][0])[2])
    assert gain > plain[0][2] - plain[1][2] > 0 and abs(lms[0, 0] - R.score_sentence(twin, plain[1][0])[2]) < 1e-3


def test_true_lengths_beyond_max_tokens(ops, pkg):
    r64, (n_hyp, ids, n_tok, *_) = check(ops, pkg, "short_ids")
    assert ids.shape[2] == 3 and n_tok[0, 0] == len(r64[0]["hyps"][0][0]) > 3


@pytest.mark.parametrize("name", ["with_hotwords", "packed_37_0_300"])
def test_no_model_is_the_sibling_bit_for_bit(ops, pkg, name):
    c = case(name)
    got = run(ops, pkg, c, with_lm=False)
    ids, lp, off, n, lens = tensors(c)
    nu = len(lens)
    graphs = [] if c.graph_words is None else [pkg.ContextGraph(c.graph_words[0], c.graph_words[1], c.V)]
    sib = ops.ctc_prefix_beam_multi(ids, lp, off, n, c.V, [c.fb] * nu, [c.sb] * nu, [c.nbest] * nu, graph_of=[0 if graphs else -1] * nu,
                                    graphs=graphs, max_tokens=max(lens))
    torch.cuda.synchronize()
    for g, w in zip(got[:6], sib):
        w = w.cpu().numpy()
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)) if w.dtype == np.float32 else np.array_equal(g, w)
    assert (got[6].view(np.uint32) == 0).all()


def test_refused_before_launch(ops, pkg):
    c = case("merge")
    ids, lp, off, n, lens = tensors(c)
    other = pkg.LmGraph.from_ngrams([((0,), -1.0, 0.0)], 4)
    with pytest.raises(pkg.PfhipError):
        ops.ctc_prefix_beam_multi_lm(ids, lp, off, n, 3, [3], [3], [3], other)                       # a model of another vocabulary
    lm = pkg.LmGraph.from_ngrams(SMALL_LM[0], 3, **SMALL_LM[1])
    for kw in (dict(first_beam=[4]), dict(second_beam=[17]), dict(nbest=[4]), dict(blank=9), dict(workspace_bytes=8)):
        a = dict(dict(first_beam=[3], second_beam=[3], nbest=[3]), **kw)
        with pytest.raises(pkg.PfhipError):
            ops.ctc_prefix_beam_multi_lm(ids, lp, off, n, 3, a.pop("first_beam"), a.pop("second_beam"), a.pop("nbest"), lm, **a)
