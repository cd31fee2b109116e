"""GPU: a token n-gram language model set on a model handle (pfhip_set_token_lm) and walked by the searches of its forwards, on the
smallest synthetic Paraformer and SenseVoice of the existing bias and beam tests.

After set_token_lm the hypotheses are the restatement's (tests/lm_ref.py) on the candidates THE SAME CALL returned: for the
Paraformer bit for bit (ids, counts, the bits of the four scores), for SenseVoice by the rule of
tests/test_gpu_ctc_prefix_beam_op.py on "ctc_topk_*" (e = the float32 / float64 distance of the restatement, every prune and final
margin of the float64 run at least 16 e, the device's hypotheses float64's in order, every score within 4 e, the model's share
included).  `out`, the detail buffers and the spans are bit for bit the plain call's; set_token_lm(None) restores the earlier results
bit for bit; a graph of another vocabulary is refused."""
import importlib
import threading

import numpy as np
import pytest

import lm_ref as R
from conftest import synth_pcm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K = 8
LM_KW = dict(scale=0.3, token_bonus=0.1, oov_log10=-4.0)
SVS_LM_SEED = 6                                  # the seed of the model's n-grams: every margin below is wide with it


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- Paraformer -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def para(pkg, weights_mod):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    man, blob = weights_mod.synth_weights(weights_mod.small_config(enc_layers=2, dec_layers=1), seed=41)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    yield m
    m.close()


@pytest.fixture(scope="module")
def para_utts():
    rng = np.random.default_rng(57)
    return [synth_pcm(0, 16000 * 1 + 123, rng), synth_pcm(1, 16000 * 2 + 7, rng), synth_pcm(2, 16000 * 3 - 55, rng)]


SETS = ((2, 8, 3), (8, 16, 16), (4, 4, 1))       # (width, beam, nbest) of the three utterances


def para_run(model, utts, graph=None, **kw):
    return model.forward_bias(utts, [s + (graph,) for s in SETS], set_of=[0, 1, 2], nbest=K, want_fire_frames=True, nbest_fill=-77, **kw)


def para_ngrams(plain, V):
    """Unigrams for most tokens, and bi- and trigrams over the candidates the head really returns, so that arcs are taken."""
    rng = np.random.default_rng(5)
    r = lambda lo, hi: round(float(rng.uniform(lo, hi)), 4)
    grams = {(w,): (r(-4, -1), r(-0.8, 0)) for w in range(V) if w % 7 != 3}
    grams[(V,)] = (r(-2, -1), 0.0)
    grams[(V + 1,)] = (-99.0, r(-0.8, 0))
    for b in range(len(plain["ids"])):
        ids, n = plain["nbest_ids"][b], len(plain["ids"][b])
        for t in range(n - 1):
            for a, c in ((0, 0), (0, 1), (1, 0), (1, 2), (2, 1)):
                g = (int(ids[t, a]), int(ids[t + 1, c]))
                if (g[0],) in grams and g not in grams:
                    grams[g] = (r(-1.5, -0.1), r(-0.5, 0))
            if t + 2 < n:
                g = (int(ids[t, 0]), int(ids[t + 1, 0]), int(ids[t + 2, 1]))
                if g[:2] in grams and g not in grams:
                    grams[g] = (r(-1, -0.1), 0.0)
    return [(g, p, b) for g, (p, b) in grams.items()]


def para_check(model, r, twin, graph=None):
    stride = max(s[2] for s in SETS)
    mt = r["bias"]["ids"].shape[2]
    lms = model.beam_lm_score(len(SETS), stride)
    dump = graph.dump() if graph is not None else None
    for b, (w, bm, nb) in enumerate(SETS):
        rows = min(int(r["token_num"][b]), int(r["n_fires"][b]))
        assert rows > 0
        hyps = R.nar_search(r["nbest_ids"][b, :rows], r["nbest_logp"][b, :rows], w, bm, nb, twin, graph=dump, vocab=model.vocab_size)
        got = tuple(r["bias"][key][b] for key in ("n_hyp", "ids", "n_tokens", "score", "am_score", "ctx_score")) + (lms[b],)
        bad = R.nar_mismatches(got, R.nar_as_outputs(hyps, stride, mt))
        assert not bad, (b, bad)
    return lms


def test_paraformer_search_walks_the_model(para, pkg, para_utts):
    V = para.vocab_size
    plain = para.forward_ids(para_utts, nbest=K, want_fire_frames=True, nbest_fill=-77)
    before = para_run(para, para_utts)
    grams = para_ngrams(plain, V)
    with pytest.raises(pkg.PfhipError) as e:
        para.set_token_lm(pkg.LmGraph.from_ngrams(grams[:50], V - 1, **LM_KW))
    assert e.value.status == 1 and "vocabulary" in str(e.value)
    with pytest.raises(pkg.PfhipError):
        para.beam_lm_score(3, 16)                                    # no search has walked a model yet
    lm = pkg.LmGraph.from_ngrams(grams, V, **LM_KW)
    twin = R.Lm(grams, V, **LM_KW)
    para.set_token_lm(lm)
    lm.close()                                                       # the image is on the device: the host graph may go
    try:
        r = para_run(para, para_utts)
        for key in ("token_num", "n_fires", "n_frames", "nbest_ids", "fire_frame"):
            assert np.array_equal(r[key], plain[key]), key
        assert same_bits(r["nbest_logp"], plain["nbest_logp"]) and all(np.array_equal(x, y) for x, y in zip(r["ids"], plain["ids"]))
        lms = para_check(para, r, twin)
        assert (lms[1] != 0).all() and not same_bits(r["bias"]["score"], before["bias"]["score"])
        # with a hotword graph beside the model
        ids2 = plain["nbest_ids"][2]
        g = pkg.ContextGraph([[int(ids2[3, 1]), int(ids2[4, 1])]], [1.5], V)
        para_check(para, para_run(para, para_utts, g), twin, g)
        # a plain forward does not read the model
        again = para.forward_ids(para_utts, nbest=K, want_fire_frames=True, nbest_fill=-77)
        assert same_bits(again["nbest_logp"], plain["nbest_logp"])
    finally:
        para.set_token_lm(None)
    after = para_run(para, para_utts)
    for key, x in before["bias"].items():
        assert same_bits(x, after["bias"][key]), key


# ---- SenseVoice -----------------------------------------------------------------------------------------------------------------------
SECONDS = (1.0, 0.02, 2.5)
KW = dict(lid=[4, 0, 3], textnorm=[14, 15, 15])


@pytest.fixture(scope="module")
def svs(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    wt = importlib.import_module("asr_2pass_amd.weights")
    m = pkg.SenseVoiceHip().InitAsr(wt.synth_svs_weights(seed=1360), device=0)
    m.set_inflight(2)
    yield m
    m.close()


@pytest.fixture(scope="module")
def svs_utts():
    out = []
    for i, seconds in enumerate(SECONDS):
        x = synth_pcm(30 + i, int(seconds * 16000), np.random.default_rng(900 + i))
        out.append(np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16))
    return out


def svs_ngrams(V, seed=SVS_LM_SEED):
    return R.random_ngrams(np.random.default_rng(seed), V, 3, [4000, 4000], missing=(V - 1, V - 2))


def same_out(got, plain):
    assert got["token_num"].tolist() == plain["token_num"].tolist() and got["frame_len"].tolist() == plain["frame_len"].tolist()
    for b in range(len(plain["ids"])):
        for key in ("ids", "tok_frame", "tok_logp", "frame_ids", "frame_logp"):
            assert same_bits(got[key][b], plain[key][b]), (key, b)


def same_beam(a, b, ua=None, ub=None):
    ua = range(len(a["beam_ids"])) if ua is None else ua
    ub = ua if ub is None else ub
    for x, y in zip(ua, ub):
        assert a["beam_n_hyp"][x] == b["beam_n_hyp"][y]
        assert [h.tolist() for h in a["beam_ids"][x]] == [h.tolist() for h in b["beam_ids"][y]]
        for key in ("beam_score", "beam_ctc_score", "beam_ctx_score"):
            assert same_bits(a[key][x], b[key][y]), (key, x)


def svs_check(model, got, lms, fb, sb, nbest, twin, what=""):
    """The search on the device's own k best columns, per utterance over its speech rows."""
    import ctc_beam_ref as C
    V, blank = int(model.cfg["vocab"]), int(model.cfg.get("blank_id", 0))
    T = [int(x) for x in got["frame_len"]]
    M = sum(T)
    ids = model.get_tensor("ctc_topk_ids", M * fb).view(np.int32).reshape(M, fb)
    lp = model.get_tensor("ctc_topk_logp", M * fb).reshape(M, fb)
    off = 0
    for b, n in enumerate(T):
        rows = slice(off + 4, off + n) if n else slice(0, 0)
        run = lambda ft: R.ctc_search(ids[rows], lp[rows], blank, fb, sb, twin, ft=ft, vocab=V, nbest=nbest)
        r64, r32 = run(np.float64), run(np.float32)
        agree = [h[0] for h in r64["hyps"]] == [h[0] for h in r32["hyps"]]
        e = max([abs(x[i] - y[i]) for x, y in zip(r64["hyps"], r32["hyps"]) for i in (1, 2, 3, 4)] + [0.0])
        print(f"{what} utterance {b}: rows {max(n - 4, 0)}  e {e:.3e}  prune margin {r64['prune_margin']:.3e}  final margin {r64['final_margin']:.3e}")
        assert agree, f"{what} utterance {b}: float32 and float64 disagree"
        assert r64["prune_margin"] >= 16 * e and r64["final_margin"] >= 16 * e, f"{what} utterance {b}: a decision closer than 16 e"
        assert got["beam_n_hyp"][b] == len(r64["hyps"])
        worst = 0.0
        for j, (toks, s, cs, cx, l) in enumerate(r64["hyps"]):
            assert got["beam_ids"][b][j].tolist() == toks, (what, b, j)
            worst = max(worst, abs(got["beam_score"][b][j] - s), abs(got["beam_ctc_score"][b][j] - cs), abs(got["beam_ctx_score"][b][j] - cx),
                        abs(lms[b][j] - l))
        assert (lms[b][len(r64["hyps"]):] == 0).all()
        print(f"{what} utterance {b}: device error {worst:.3e}  bound {4 * e:.3e}")
        assert worst <= 4 * e
        off += n


def test_sensevoice_search_walks_the_model(svs, pkg, svs_utts):
    V = int(svs.cfg["vocab"])
    plain = svs.forward(svs_utts, **KW)
    before = svs.forward(svs_utts, beam=(5, 5), nbest=3, **KW)
    spans_before = svs.forward([svs_utts[2]], lid=[3], textnorm=[15], want_spans=True)
    grams = svs_ngrams(V)
    with pytest.raises(pkg.PfhipError):
        svs.set_token_lm(pkg.LmGraph.from_ngrams(grams[:50], V + 1, **LM_KW))
    lm, twin = pkg.LmGraph.from_ngrams(grams, V, **LM_KW), R.Lm(grams, V, **LM_KW)
    svs.set_token_lm(lm)
    lm.close()
    try:
        got = svs.forward(svs_utts, beam=(5, 5), nbest=3, **KW)
        lms = svs.beam_lm_score(3, 3)
        same_out(got, plain)
        svs_check(svs, got, lms, 5, 5, 3, twin, what="beam 5/5")
        assert got["beam_n_hyp"].tolist() == [3, 0, 3] and (lms[1] == 0).all() and (lms[2] != 0).all()
        assert not same_bits(got["beam_score"][2], before["beam_score"][2])
        # the sets form: every utterance on the lone call's set, and one left out
        sets = svs.forward(svs_utts, beam_sets=[(5, 5, 3, None), None, (5, 5, 3, None)], **KW)
        same_out(sets, plain)
        same_beam(sets, got, (0, 2))
        assert same_bits(svs.beam_lm_score(3, 3), lms) and sets["beam_n_hyp"][1] == 0
        # a greedy forward, and one with spans, do not read the model
        same_out(svs.forward(svs_utts, **KW), plain)
        with pytest.raises(pkg.PfhipError):
            svs.beam_lm_score(3, 3)                                  # the tensor lives until the context's next forward, searching or not
        spans = svs.forward(svs_utts, want_spans=True, **KW)
        same_out(spans, plain)
        sp1 = svs.forward([svs_utts[2]], lid=[3], textnorm=[15], want_spans=True)
        for key in ("span_begin", "span_end", "span_logp"):
            assert same_bits(sp1[key][0], spans_before[key][0]), key
        assert same_bits(sp1["span_score"], spans_before["span_score"])

        # merged beam callers on two threads: each gets its lone call's hypotheses.  A packed forward's rows differ from a lone
        # forward's in the last bits (tests/test_gpu_sensevoice_merge.py: log-probs within 1e-4 a row), so the scores are compared
        # within 1e-4 a speech row; the model's share depends on the tokens alone and is the lone call's bit for bit
        # A third caller asks for the spans of its greedy tokens: in a merged forward spans, searches and the model share one
        # head, and the spans must stay those of the caller's lone forward WITHOUT a model (ids and spans exactly, log-probs within
        # 1e-4, the rule of tests/test_gpu_sensevoice_merge.py)
        calls = [(0, 3), (2, 2)]                                     # (utterance, nbest) of the two beam callers
        one = lambda u, nb: svs.forward([svs_utts[u]], lid=[KW["lid"][u]], textnorm=[KW["textnorm"][u]], beam=(5, 5), nbest=nb)
        lone = []
        for u, nb in calls:
            r = one(u, nb)
            lone.append((r, svs.beam_lm_score(1, nb)))
        svs.set_batching(200000, 8)
        svs.set_beam_merging(True)
        res, errs, barrier = [None, None, None], [], threading.Barrier(3)

        def caller(k):
            try:
                barrier.wait()
                if k == 2:
                    res[k] = svs.forward([svs_utts[2]], lid=[3], textnorm=[15], want_spans=True)
                    return
                r = one(*calls[k])
                res[k] = (r, svs.beam_lm_score(1, calls[k][1]))
            except Exception as ex:                                  # noqa: BLE001 — reported by the main thread
                errs.append(ex)

        th = [threading.Thread(target=caller, args=(k,)) for k in range(3)]
        [t.start() for t in th]
        [t.join() for t in th]
        svs.set_beam_merging(False)
        svs.set_batching(0)
        assert not errs, errs
        for k in range(2):
            (r, l), (r0, l0) = res[k], lone[k]
            tol = 1e-4 * max(int(r0["frame_len"][0]) - 4, 1)
            assert r["beam_n_hyp"].tolist() == r0["beam_n_hyp"].tolist() == [calls[k][1]]
            assert [h.tolist() for h in r["beam_ids"][0]] == [h.tolist() for h in r0["beam_ids"][0]], k
            for key in ("beam_score", "beam_ctc_score", "beam_ctx_score"):
                assert np.abs(r[key][0] - r0[key][0]).max() <= tol, (k, key)
            assert same_bits(l, l0), k
        sp = res[2]
        assert sp["ids"][0].tolist() == spans_before["ids"][0].tolist()
        for key in ("span_begin", "span_end"):
            assert sp[key][0].tolist() == spans_before[key][0].tolist(), key
        assert np.abs(sp["span_logp"][0] - spans_before["span_logp"][0]).max() <= 1e-4
        assert abs(sp["span_score"][0] - spans_before["span_score"][0]) <= 1e-4 * max(int(sp["frame_len"][0]) - 4, 1)
    finally:
        svs.set_batching(0)
        svs.set_token_lm(None)
    after = svs.forward(svs_utts, beam=(5, 5), nbest=3, **KW)
    same_out(after, plain)
    same_beam(after, before)
    with pytest.raises(pkg.PfhipError):
        svs.beam_lm_score(3, 3)                                      # the last search walked no model
