"""GPU: the beam search over a non-autoregressive head's candidates with a token n-gram language model fused in (csrc/nar_beam.hip,
the kLm instantiation) through pfhip_op_nbest_ctx_beam_lm, against the restatement tests/lm_ref.py (which tests/test_lm_ref.py holds
to brute force).  Ids, counts and the bits of all four scores (total, am, context, lm) are EQUAL: every sum is a single fp32 add in
a stated order, so no tolerance applies."""
import functools
import importlib

import numpy as np
import pytest

import lm_ref as R
import nar_beam_ref as N

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V, K = N.V, N.K


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


@functools.lru_cache(maxsize=None)
def model_ngrams(seed=1, order=3):
    return tuple(R.random_ngrams(np.random.default_rng(seed), V, order, [900, 1200, 600][:order - 1], missing=(7, 40)))


def pack(utts):
    ids = np.concatenate([x[0] for x in utts] + [np.zeros((1, K), np.int32)]).astype(np.int32)
    lp = np.concatenate([x[1] for x in utts] + [np.zeros((1, K), np.float32)]).astype(np.float32)
    lens = [len(x[0]) for x in utts]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    return (torch.from_numpy(ids).cuda(), torch.from_numpy(lp).cuda(), torch.from_numpy(offs).cuda(),
            torch.tensor(lens, dtype=torch.int32).cuda(), sum(lens))


def launch(ops, utts, desc, lm, graphs=(), graph_of=None, max_tokens=None):
    ids, lp, off, n, rows = pack(utts)
    mt = max(len(u[0]) for u in utts) if max_tokens is None else max_tokens
    out = ops.nbest_ctx_beam_lm(ids, lp, off, n, V, [d[0] for d in desc], [d[1] for d in desc], [d[2] for d in desc], lm,
                                graph_of=graph_of, graphs=graphs, max_tokens=mt, rows=rows)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out], mt


def check(ops, pkg, utts, desc, grams, lm_kw, words=None, graph_of=None, max_tokens=None):
    lm = pkg.LmGraph.from_ngrams(list(grams), V, **lm_kw)
    twin = R.Lm(list(grams), V, **lm_kw)
    graphs = [pkg.ContextGraph(w[0], w[1], V) for w in (words or [])]
    dumps = [g.dump() for g in graphs]
    graph_of = [-1] * len(utts) if graph_of is None else list(graph_of)
    out, mt = launch(ops, utts, desc, lm, graphs, graph_of, max_tokens)
    stride = max(d[2] for d in desc)
    hyps = []
    for b, ((ids, lp), (w, bm, nb), g) in enumerate(zip(utts, desc, graph_of)):
        h = R.nar_search(ids, lp, w, bm, nb, twin, graph=None if g < 0 else dumps[g], vocab=V)
        want = R.nar_as_outputs(h, stride, mt)
        got = tuple(t[b] for t in out)
        assert R.nar_mismatches(got, want) == [], (b, R.nar_mismatches(got, want), got, want)
        hyps.append(h)
    return hyps, out


LM_KW = dict(scale=0.4, token_bonus=0.2, oov_log10=-5.0)


def test_every_slot_live(ops, pkg):
    """Width 8 x beam 16 over 13 rows: from the third row on all 128 (hypothesis, candidate) pairs are live."""
    hyps, _ = check(ops, pkg, [N._rows("random", 13, 3)], [(8, 16, 16)], model_ngrams(), LM_KW)
    assert len(hyps[0]) == 16 and len({tuple(h[0]) for h in hyps[0]}) == 16 and any(h[4] != 0 for h in hyps[0])


def test_width_one_beam_one(ops, pkg):
    utt = N._rows("random", 9, 5)
    hyps, out = check(ops, pkg, [utt], [(1, 1, 1)], model_ngrams(), LM_KW)
    twin = R.Lm(list(model_ngrams()), V, **LM_KW)
    assert hyps[0][0][0] == utt[0][:, 0].tolist() and out[6][0, 0] == R.score_sentence(twin, utt[0][:, 0])[2]


@pytest.mark.parametrize("kind", ["random", "ties", "dirty"])
def test_three_utterances_on_their_own_parameters(ops, pkg, kind):
    """Rows 37, 0 and 60 in one launch; ties: many totals exactly equal before the model; dirty: a NaN, a -inf, ids out of range."""
    utts = [N._rows(kind, 37, 11), N._rows(kind, 0, 12), N._rows(kind, 60, 13)]
    hyps, out = check(ops, pkg, utts, [(3, 4, 2), (8, 16, 16), (5, 7, 7)], model_ngrams(), LM_KW, max_tokens=40)
    assert out[0].tolist() == [2, 0, 7] and (out[6][1] == 0).all() and out[2][2, 0] == 60


@pytest.mark.parametrize("order", [2, 4])
def test_model_and_context_graph_together(ops, pkg, order):
    utts = N.op_utterances("random")
    one, five = N.op_words(utts)
    hyps, out = check(ops, pkg, utts, N.DESC, model_ngrams(2, order), LM_KW, words=[one, five], graph_of=(-1, 0, 1, 1), max_tokens=max(N.LENS))
    assert any(h[3] != 0 for h in hyps[3]) and any(h[4] != 0 for h in hyps[3])


def test_no_model_is_the_sibling_bit_for_bit(ops, pkg):
    utts = N.op_utterances("random")
    one, five = N.op_words(utts)
    graphs = [pkg.ContextGraph(w[0], w[1], V) for w in (one, five)]
    out, mt = launch(ops, utts, N.DESC, None, graphs, [-1, 0, 1, 0], max_tokens=max(N.LENS))
    ids, lp, off, n, rows = pack(utts)
    sib = ops.nbest_ctx_beam(ids, lp, off, n, V, [d[0] for d in N.DESC], [d[1] for d in N.DESC], [d[2] for d in N.DESC], graph_of=[-1, 0, 1, 0],
                             graphs=graphs, max_tokens=mt, rows=rows)
    torch.cuda.synchronize()
    for g, w in zip(out[:6], sib):
        w = w.cpu().numpy()
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)) if w.dtype == np.float32 else np.array_equal(g, w)
    assert (out[6].view(np.uint32) == 0).all()


def test_a_weightless_model_changes_nothing(ops, pkg):
    """scale = 0 and token_bonus = 0: every weight is +0, so ids and score are the search's without a model and lm_score is 0."""
    utts = [N._rows("random", 13, 3), N._rows("ties", 7, 4)]
    desc = [(8, 16, 16), (3, 4, 4)]
    hyps, out = check(ops, pkg, utts, desc, model_ngrams(), dict(scale=0.0, token_bonus=0.0))
    for b, ((ids, lp), (w, bm, nb)) in enumerate(zip(utts, desc)):
        plain = N.search(ids, lp, w, bm, nb)
        assert [h[0] for h in hyps[b]] == [p[0] for p in plain]
        assert [np.float32(h[1]).tobytes() for h in hyps[b]] == [np.float32(p[1]).tobytes() for p in plain]
    assert (out[6].view(np.uint32) == 0).all()


def test_the_model_flips_the_best_hypothesis(ops, pkg):
    """Without the model the greedy sequence wins; a bigram the model likes puts row 4's runner-up in front."""
    utt = N._rows("random", 9, 21)
    plain = N.search(utt[0], utt[1], 4, 8, 8)
    greedy = utt[0][:, 0].tolist()
    assert plain[0][0] == greedy
    prev, up = greedy[3], int(utt[0][4, 1])
    grams = [((w,), -1.5, -0.1) for w in range(V)] + [((V,), -1.5, 0.0), ((V + 1,), -99.0, -0.1), ((prev, up), -0.01, -0.1)]
    hyps, out = check(ops, pkg, [utt], [(4, 8, 8)], tuple(grams), dict(scale=1.0, token_bonus=0.0))
    want = greedy[:4] + [up] + greedy[5:]
    assert hyps[0][0][0] == want and out[1][0, 0, :9].tolist() == want
    assert float(plain[0][2]) > float(hyps[0][0][2])                 # it won on the model's share, not on the acoustic score


def test_refused_before_launch(ops, pkg):
    utt = N._rows("random", 5, 1)
    other = pkg.LmGraph.from_ngrams([((0,), -1.0, 0.0)], V - 1)
    with pytest.raises(pkg.PfhipError):
        launch(ops, [utt], [(4, 8, 8)], other)                       # a model of another vocabulary
    with pytest.raises(pkg.PfhipError):
        launch(ops, [utt], [(9, 8, 8)], pkg.LmGraph.from_ngrams([((0,), -1.0, 0.0)], V))
