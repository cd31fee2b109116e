"""GPU: the CTC prefix beam search with hotwords (csrc/ctc_beam.hip) through pfhip_op_ctc_prefix_beam on hand-made [rows][k] arrays
(no GEMM), against the plain-Python restatement tests/ctc_beam_ref.py (which tests/test_ctc_beam_ref.py holds to brute force).

Rule of every comparison: let e be the largest difference between the restatement run in float32 and in float64 over the scores of
the case (total, ctc and context score of every returned hypothesis).  The device's hypotheses must be the float64 restatement's, in
order, with every score within 4 e — the project's bound for fp32-grade arithmetic (tests/test_gpu_dnsmos_ops.py).  Which
hypotheses survive is only well defined where no decision is closer than the arithmetic's error, so each case first asserts that
every prune margin (last kept - first dropped total, every frame) and every margin of the final order of the float64 run is at
least 16 e.  A failure of THAT assertion means "choose another seed", not "kernel bug"; the seeds below were chosen on the CPU.
Rows hold float32 values, so both runs and the device read the same numbers.  e, the margins and the device's error are printed."""
import functools
import importlib

import numpy as np
import pytest

import ctc_beam_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

A, B = 1, 2


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def rows_of(logp_full, k):
    """The k best columns of every row of a full [T][V] log-probability matrix, best first, lower column first among equals."""
    logp_full = np.asarray(logp_full, np.float64)
    ids = np.argsort(-logp_full, axis=1, kind="stable")[:, :k]
    return ids.astype(np.int32), np.take_along_axis(logp_full, ids, axis=1).astype(np.float32)


def random_rows(T, V, k, seed, conc=0.3):
    rng = np.random.default_rng(seed)
    return rows_of(np.log(rng.dirichlet(np.ones(V) * conc, size=T) + 1e-12), k)


def random_words(n, V, seed):
    rng = np.random.default_rng(seed)
    words = [[int(t) for t in rng.integers(1, V, size=rng.integers(2, 7))] for _ in range(n)]
    return words, [float(rng.integers(1, 9)) / 4 for _ in words]


class Case:
    """utts: a list of (ids [T][k], logp [T][k]); graph_words: (words, weights) or None."""

    def __init__(self, utts, V, fb, sb, nbest=None, graph_words=None, max_tokens=None):
        self.utts, self.V, self.fb, self.sb = utts, V, fb, sb
        self.nbest = sb if nbest is None else nbest
        self.graph_words, self.max_tokens = graph_words, max_tokens

    def twin(self):
        if self.graph_words is None:
            return None
        words, per_word = self.graph_words
        return R.Graph(words, [[w] * len(x) for x, w in zip(words, per_word)], self.V)

    def oracle(self, ft):
        g = self.twin()
        return [R.search(i, l, 0, self.fb, self.sb, graph=g, ft=ft, vocab=self.V, nbest=self.nbest) for i, l in self.utts]


P3 = np.log(np.array([[.5, .3, .2], [.4, .25, .35], [.6, .2, .2]]))
PM = np.log(np.array([[.1, .6, .3], [.2, .15, .65], [.25, .2, .55]]))     # [a b] arrives as an extension and is live already


def hand(P, k=None):
    P = np.asarray(P, np.float64)
    return rows_of(P, P.shape[1] if k is None else k)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "known":
        return Case([hand(P3)], 3, 3, 3)
    if name == "known_hotword":
        return Case([hand(P3)], 3, 3, 3, graph_words=([[B, A]], [1.0]))
    if name == "a_a":                            # a a -> [a]; a blank a -> [a a]
        return Case([hand(np.log([[.1, .8, .1], [.15, .8, .05]])), hand(np.log([[.1, .8, .1], [.8, .15, .05], [.2, .7, .1]]))], 3, 3, 3)
    if name == "merge":
        return Case([hand(PM)], 3, 3, 8, nbest=3)
    if name == "blank_outside_topk":             # k = 2 of 6 columns: in most rows the blank is no candidate and an unchanged
        return Case([random_rows(30, 6, 2, 3, conc=1.0)], 6, 2, 4)   # hypothesis lives on only through a repeat
    if name == "beam_1_1":
        return Case([random_rows(40, 6, 1, 11)], 6, 1, 1)
    if name == "beam_16_16":
        return Case([random_rows(12, 24, 16, 21, conc=2.0)], 24, 16, 16, nbest=4)
    if name == "one_frame":
        return Case([random_rows(1, 9, 4, 2, conc=1.0)], 9, 4, 4)
    if name == "packed_37_0_300":
        # peaked rows keep the long utterance's score near -50, where an fp32 step is 4e-6: the margins stay wide against e
        return Case([random_rows(37, 50, 5, 101, conc=.02), random_rows(0, 50, 5, 0), random_rows(300, 50, 5, 106, conc=.005)], 50, 5, 5,
                    nbest=3)
    if name == "short_ids":
        return Case([random_rows(40, 50, 5, 7)], 50, 5, 5, nbest=2, max_tokens=3)
    base = random_rows(40, 50, 5, 7)
    plain = R.search(base[0], base[1], 0, 5, 5, vocab=50)["hyps"]
    best, second = plain[0][0], plain[1][0]
    if name == "hotword_flip":                   # the runner-up as a hotword: it overtakes the best
        return Case([base], 50, 5, 5, graph_words=([second], [1.5]))
    if name == "hotword_escape":                 # token 1 starts the hotword [1 2], token 3 leaves it: the bonus is taken back
        return Case([hand(np.log([[.05, .8, .05, .1], [.05, .05, .1, .8], [.7, .1, .1, .1]]))], 4, 4, 4, nbest=3, graph_words=([[1, 2]], [0.5]))
    if name == "hotword_cut_off":                # a hotword whose last token never comes: the match is open at the end
        other = next(t for t in range(1, 50) if t not in best)
        return Case([base], 50, 5, 5, graph_words=([best[-2:] + [other]], [0.25]))
    if name == "hotword_prefix_pair":
        return Case([base], 50, 5, 5, graph_words=([best[:2], best[:3], best[1:3]], [0.5, 0.25, 0.75]))
    if name == "hotword_200":
        words, weights = random_words(200, 50, 9)
        return Case([base], 50, 5, 5, graph_words=(words + [second[:3]], weights + [1.0]))
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
            e = max(e, max(abs(x[i] - y[i]) for i in (1, 2, 3)))
        prune, final = min(prune, a["prune_margin"]), min(final, a["final_margin"])
    return r64, e, prune, final


def run(ops, pkg, c):
    k = c.utts[0][0].shape[1]
    ids = np.concatenate([u[0] for u in c.utts]).reshape(-1, k)
    lp = np.concatenate([u[1] for u in c.utts]).reshape(-1, k)
    lens = [len(u[0]) for u in c.utts]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    pad = lambda a, dt: torch.from_numpy(np.concatenate([a, np.zeros((1, k), dt)]).astype(dt)).cuda()      # never an empty tensor
    graph = None if c.graph_words is None else pkg.ContextGraph(c.graph_words[0], c.graph_words[1], c.V)
    mt = max(lens) if c.max_tokens is None else c.max_tokens
    out = ops.ctc_prefix_beam(pad(ids, np.int32)[:len(ids)], pad(lp, np.float32)[:len(ids)], torch.from_numpy(offs).cuda(),
                              torch.tensor(lens, dtype=torch.int32).cuda(), c.V, c.fb, c.sb, nbest=c.nbest, max_tokens=mt, graph=graph)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def check(ops, pkg, name):
    c = case(name)
    r64, e, prune, final = reference(name)
    print(f"{name}: e {e:.3e}  least prune margin {prune:.3e}  least final margin {final:.3e}")
    assert prune >= 16 * e and final >= 16 * e, f"{name}: a decision closer than 16 e — choose another seed"
    n_hyp, ids, n_tok, score, ctc, ctx = run(ops, pkg, c)
    mt = ids.shape[2]
    worst = 0.0
    for b, r in enumerate(r64):
        want = r["hyps"]
        assert n_hyp[b] == len(want), (name, b, n_hyp[b], len(want))
        for j, (toks, s, cs, cx) in enumerate(want):
            assert n_tok[b, j] == len(toks), (name, b, j)
            assert ids[b, j, :min(len(toks), mt)].tolist() == toks[:mt], (name, b, j)
            assert (ids[b, j, len(toks):] == -1).all()
            worst = max(worst, abs(score[b, j] - s), abs(ctc[b, j] - cs), abs(ctx[b, j] - cx))
        assert (n_tok[b, len(want):] == 0).all() and (ids[b, len(want):] == -1).all() and np.isneginf(score[b, len(want):]).all()
    print(f"{name}: device error {worst:.3e}  bound {4 * e:.3e}")
    assert worst <= 4 * e, (name, worst, 4 * e)
    return r64, (n_hyp, ids, n_tok, score, ctc, ctx)


@pytest.mark.parametrize("name", ["known", "known_hotword"])
def test_known_answers(ops, pkg, name):
    """Three frames of (blank, a, b): [b] ln .284, [a] ln .272, [] ln .12; with the hotword [b a] at 1 a token [b a] (ctc ln .105,
    context 2), then [b] at ln .244 after the final back-off, then [a]."""
    r64, _ = check(ops, pkg, name)
    want = [[B], [A], []] if name == "known" else [[B, A], [B], [A]]
    assert [h[0] for h in r64[0]["hyps"]] == want


@pytest.mark.parametrize("name", ["a_a", "merge", "blank_outside_topk"])
def test_repeat_blank_and_merge(ops, pkg, name):
    """a a -> [a] and a blank a -> [a a]; an extension that names a live hypothesis is added to it, not listed twice; with the blank
    outside the k best an unchanged hypothesis vanishes unless its last token repeats."""
    r64, (n_hyp, ids, n_tok, *_) = check(ops, pkg, name)
    if name == "a_a":
        assert r64[0]["hyps"][0][0] == [A] and r64[1]["hyps"][0][0] == [A, A]
    for b in range(len(r64)):
        seqs = [tuple(ids[b, j, :n_tok[b, j]]) for j in range(n_hyp[b])]
        assert len(set(seqs)) == len(seqs)


def test_beam_one_is_the_collapse_of_the_argmax(ops, pkg):
    r64, _ = check(ops, pkg, "beam_1_1")
    assert r64[0]["hyps"][0][0] == R.collapse(case("beam_1_1").utts[0][0][:, 0].tolist())


@pytest.mark.parametrize("name", ["beam_16_16", "one_frame", "packed_37_0_300"])
def test_widths_and_packing(ops, pkg, name):
    """16/16: all 256 (hypothesis, candidate) pairs are live from the fourth frame on.  One frame.  Three utterances of 37, 0 and
    300 rows in one launch: the rowless one has no hypothesis."""
    r64, (n_hyp, *_) = check(ops, pkg, name)
    if name == "packed_37_0_300":
        assert n_hyp.tolist() == [3, 0, 3]


def test_true_lengths_beyond_max_tokens(ops, pkg):
    r64, (n_hyp, ids, n_tok, *_) = check(ops, pkg, "short_ids")
    assert ids.shape[2] == 3 and n_tok[0, 0] == len(r64[0]["hyps"][0][0]) > 3


@pytest.mark.parametrize("name", ["hotword_flip", "hotword_escape", "hotword_cut_off", "hotword_prefix_pair", "hotword_200"])
def test_hotwords(ops, pkg, name):
    r64, (n_hyp, ids, n_tok, score, ctc, ctx) = check(ops, pkg, name)
    plain = reference("short_ids")[0][0]["hyps"]                     # the same rows without a graph
    if name == "hotword_flip":
        assert r64[0]["hyps"][0][0] == plain[1][0] and ctx[0, 0] > 0
    if name == "hotword_escape":                                     # what the first token earned is taken back: no bonus is left
        assert r64[0]["hyps"][0][0] == [1, 3] and ctx[0, 0] == 0
        assert [1, 2] in [h[0] for h in r64[0]["hyps"]]              # the completed hotword is a hypothesis too, with its bonus
    if name == "hotword_cut_off":
        assert r64[0]["hyps"][0][3] == 0 and ctx[0, 0] == 0


def test_refused_before_launch(ops, pkg):
    ids, lp = (torch.zeros((4, 3), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32))
    off, n = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.full((1,), 4, dtype=torch.int32, device="cuda")
    for kw in (dict(first_beam=4, second_beam=3), dict(first_beam=0, second_beam=3), dict(first_beam=3, second_beam=17),
               dict(first_beam=3, second_beam=3, nbest=4), dict(first_beam=3, second_beam=3, blank=9),
               dict(first_beam=3, second_beam=3, workspace_bytes=8)):
        with pytest.raises(pkg.PfhipError):
            ops.ctc_prefix_beam(ids, lp, off, n, 9, **kw)
    with pytest.raises(pkg.PfhipError):
        ops.ctc_prefix_beam(ids, lp, off, n, 9, 3, 3, graph=pkg.ContextGraph([[1, 2]], [1.0], 8))      # another vocabulary


def test_untrusted_rows_stay_inside(ops, pkg):
    """Ids outside 0 .. V - 1, NaN and infinite log-probabilities, and an utterance whose rows leave the array the kernel is told of:
    the outputs are well formed (ids inside the vocabulary, lengths within the rows) and the refused utterance has no hypothesis.
    The tensors hold 80 rows and the workspace is sized for 80 while the kernel is told 64, so the third utterance's rows 60 .. 68
    lie in memory this test owns whatever the kernel does with them."""
    rng = np.random.default_rng(5)
    ids = rng.integers(-2 ** 31, 2 ** 31 - 1, size=(80, 4)).astype(np.int32)
    lp = rng.standard_normal((80, 4)).astype(np.float32)
    lp[::3, 0] = np.nan; lp[1::5, 1] = -np.inf; lp[2::7, 2] = np.inf
    off = torch.tensor([0, 40, 60], dtype=torch.int32).cuda()
    n = torch.tensor([40, 20, 9], dtype=torch.int32).cuda()          # the third would end at row 69 of 64
    n_hyp, out, n_tok, score, ctc, ctx = ops.ctc_prefix_beam(torch.from_numpy(ids).cuda(), torch.from_numpy(lp).cuda(), off, n, 30, 4, 8,
                                                             nbest=8, max_tokens=40, rows=64)
    torch.cuda.synchronize()
    n_hyp, out, n_tok = n_hyp.cpu().numpy(), out.cpu().numpy(), n_tok.cpu().numpy()
    assert n_hyp[2] == 0 and 1 <= n_hyp[0] <= 8 and 1 <= n_hyp[1] <= 8
    for b, T in ((0, 40), (1, 20)):
        for j in range(n_hyp[b]):
            assert 0 <= n_tok[b, j] <= T
            assert ((out[b, j, :n_tok[b, j]] >= 0) & (out[b, j, :n_tok[b, j]] < 30)).all()
