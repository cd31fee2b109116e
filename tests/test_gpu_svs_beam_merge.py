"""GPU: SenseVoice beam callers in the merge queue (SenseVoiceHip.set_beam_merging = pfhip_svs_set_beam_merging, on top of
set_batching): greedy callers and beam callers with their own beams and hotword graphs share packed forwards — one head launch at
the largest first_beam, one search launch with every utterance on its caller's parameters.

Six threads behind one barrier, two execution contexts, a 200-ms window, utterances of 0.02-2.5 s: two greedy callers (one with
spans), four beam callers with different beams and different one-word graphs — one with two utterances of which one has no rows,
one in the sets form with a set per utterance, one with 16-bit samples.

What a caller gets in `out` is compared with its lone call by the rule of tests/test_gpu_sensevoice_merge.py: ids, frames and spans
exactly, log-probs within LOGP_TOL = 1e-4.  A beam caller's hypotheses are compared with the plain-Python restatement
(tests/ctc_beam_ref.py) on ITS OWN k best columns of the forward that served it (pfhip_get_tensor "ctc_topk_*" returns the calling
thread's rows, pfhip_debug_poke "svs_topk_k" their stride), by the rule of tests/test_gpu_ctc_prefix_beam_op.py: e = the float32 /
float64 distance of the restatement, every prune and final margin of the float64 run at least 16 e (else: another weight seed), the
device's hypotheses float64's in order, scores within 4 e."""
import importlib
import threading

import numpy as np
import pytest

import ctc_beam_ref as R
from conftest import synth_pcm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LOGP_TOL = 1e-4
WAIT_US, MAX_UTTS = 200000, 8
# per caller: seconds of its utterances, language, ITN, 16-bit samples, kind, per utterance (first_beam, second_beam, nbest, hotword?)
CALLERS = [((0.3, 1.1), "zh", True, False, "spans", None),
           ((2.5,), "en", False, False, "greedy", None),
           ((0.02, 0.9), "auto", True, False, "beam", [(3, 3, 3, True)] * 2),
           ((1.6,), "ja", False, True, "beam", [(5, 5, 2, True)]),
           ((0.7, 2.1), "ko", True, False, "sets", [(10, 10, 4, True), (3, 5, 2, False)]),
           ((0.5,), "yue", False, False, "beam", [(1, 1, 1, True)])]
BEAM = [k for k, c in enumerate(CALLERS) if c[5] is not None]


@pytest.fixture(scope="module")
def model(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    wt = importlib.import_module("asr_2pass_amd.weights")
    m = pkg.SenseVoiceHip().InitAsr(wt.synth_svs_weights(seed=1360), device=0)
    m.set_inflight(2)
    yield m
    m.close()


@pytest.fixture(scope="module")
def audio():
    out = []
    for k, c in enumerate(CALLERS):
        utts = []
        for i, sec in enumerate(c[0]):
            x = synth_pcm(10 * k + i, int(round(sec * 16000)), np.random.default_rng(7000 + 10 * k + i))
            utts.append(np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16) if c[3] else x.astype(np.float32))
        out.append(utts)
    return out


@pytest.fixture(scope="module")
def graphs(pkg, model, audio):
    """Per beam caller its one-word graph (ContextGraph, twin): the first two tokens (or the only one) of the best hypothesis of its longest
    utterance's plain search.  The synthetic weights give most callers the same leading tokens, so the graphs differ in the word's
    weight — 0.5, 0.75, 1.0, 1.25 a token, exact in binary —: four graphs of four contents, none shared in the bank."""
    V = int(model.cfg["vocab"])
    out, words = {}, []
    for i, k in enumerate(BEAM):
        c = CALLERS[k]
        u = int(np.argmax(c[0]))
        fb, sb, nb, _ = c[5][u]
        best = model.forward(audio[k], lang=c[1], itn=c[2], beam=(fb, sb), nbest=nb)["beam_ids"][u][0].tolist()
        word, weight = best[:2], 0.5 + 0.25 * i
        assert len(word) >= 1
        out[k] = (pkg.ContextGraph([word], [weight], V), R.Graph([word], [[weight] * len(word)], V))
        words.append((tuple(word), weight))
    assert len(set(words)) == len(words)
    yield out
    for g, _ in out.values():
        g.close()


def call(model, audio, graphs, k, **kw):
    c = CALLERS[k]
    if c[4] == "spans":
        return model.forward(audio[k], lang=c[1], itn=c[2], want_spans=True, **kw)
    if c[4] == "greedy":
        return model.forward(audio[k], lang=c[1], itn=c[2], **kw)
    if c[4] == "beam":
        fb, sb, nb, _ = c[5][0]
        return model.forward(audio[k], lang=c[1], itn=c[2], beam=(fb, sb), nbest=nb, graph=graphs[k][0], **kw)
    return model.forward(audio[k], lang=c[1], itn=c[2], beam_sets=[(fb, sb, nb, graphs[k][0] if hw else None) for fb, sb, nb, hw in c[5]], **kw)


@pytest.fixture(scope="module")
def alone(model, audio, graphs):
    """Every caller's call made alone, merging off: computed once, shared, left unchanged."""
    model.set_batching(0, MAX_UTTS)
    model.set_beam_merging(False)
    return [call(model, audio, graphs, k) for k in range(len(CALLERS))]


def in_threads(n, work):
    gate, res, errs = threading.Barrier(n), [None] * n, [None] * n

    def body(k):
        try:
            gate.wait(timeout=60)
            res[k] = work(k)
        except BaseException as e:                      # noqa: BLE001 — handed to the test's thread
            errs[k] = e

    ts = [threading.Thread(target=body, args=(k,)) for k in range(n)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts)
    for e in errs:
        if e is not None:
            raise e
    return res


def totals(model):
    st = model.inflight_stats()
    return sum(s["forwards"] for s in st), sum(s["calls"] for s in st)


def compare(got, ref, worst):
    assert got["token_num"].tolist() == ref["token_num"].tolist() and got["frame_len"].tolist() == ref["frame_len"].tolist()
    for b in range(len(ref["ids"])):
        for key in ("ids", "tok_frame", "frame_ids"):
            assert got[key][b].tolist() == ref[key][b].tolist(), (key, b)
        for key in ("frame_logp", "tok_logp"):
            if len(ref[key][b]):
                worst[0] = max(worst[0], float(np.abs(got[key][b] - ref[key][b]).max()))
        if "span_begin" in ref:
            assert got["span_begin"][b].tolist() == ref["span_begin"][b].tolist(), b
            assert got["span_end"][b].tolist() == ref["span_end"][b].tolist(), b
            fin = np.isfinite(ref["span_logp"][b])
            assert np.isfinite(got["span_logp"][b]).tolist() == fin.tolist()
            if fin.any():
                worst[0] = max(worst[0], float(np.abs(got["span_logp"][b][fin] - ref["span_logp"][b][fin]).max()))
            sg, sr = float(got["span_score"][b]), float(ref["span_score"][b])
            assert np.isfinite(sg) == np.isfinite(sr)
            if np.isfinite(sr):
                worst[1] = max(worst[1], abs(sg - sr))


def own_columns(model, r):
    """In the caller's thread, right behind its forward: (stride, ids, logp) of its own rows, or None where its execution context
    has run another forward since (then the read-out is that forward's, told by the size or by rank 0)."""
    k = model.debug_poke("svs_topk_k")
    rows = int(sum(r["frame_len"]))
    try:
        ids = model.get_tensor("ctc_topk_ids", 4096 * 16).view(np.int32)
        lp = model.get_tensor("ctc_topk_logp", 4096 * 16)
    except RuntimeError as e:                           # PfhipError: that later forward was a greedy one and left no columns at all
        assert getattr(e, "status", None) == 1 and "ctc_topk" in str(e), str(e)
        return None
    if k < 1 or len(ids) != rows * k or len(lp) != rows * k:
        return None
    ids, lp = ids.reshape(rows, k).copy(), lp.reshape(rows, k).copy()
    if ids[:, 0].tolist() != np.concatenate(r["frame_ids"]).tolist() or lp[:, 0].tobytes() != np.concatenate(r["frame_logp"]).tobytes():
        return None
    return k, ids, lp


def check_hypotheses(model, k, r, cols, twin, what):
    """Caller k's hypotheses against the restatement on the first first_beam columns of its own rows, from row 4 of an utterance on."""
    V, blank = int(model.cfg["vocab"]), int(model.cfg.get("blank_id", 0))
    stride, ids, lp = cols
    off = 0
    for b, n in enumerate(int(x) for x in r["frame_len"]):
        fb, sb, nbest, hw = CALLERS[k][5][b]
        assert stride >= fb
        rows = slice(off + 4, off + n) if n else slice(0, 0)
        run = lambda ft: R.search(ids[rows, :fb], lp[rows, :fb], blank, fb, sb, graph=twin if hw else None, ft=ft, vocab=V, nbest=nbest)
        r64, r32 = run(np.float64), run(np.float32)
        assert [h[0] for h in r64["hyps"]] == [h[0] for h in r32["hyps"]], f"{what} caller {k} utterance {b}: float32 and float64 disagree"
        e = max([abs(x[i] - y[i]) for x, y in zip(r64["hyps"], r32["hyps"]) for i in (1, 2, 3)] + [0.0])
        print(f"{what} caller {k} utterance {b}: stride {stride} rows {max(n - 4, 0)}  e {e:.3e}  prune margin {r64['prune_margin']:.3e}  "
              f"final margin {r64['final_margin']:.3e}")
        assert r64["prune_margin"] >= 16 * e and r64["final_margin"] >= 16 * e, f"{what} caller {k} utterance {b}: a decision closer than 16 e"
        assert r["beam_n_hyp"][b] == len(r64["hyps"])
        worst = 0.0
        for j, (toks, s, cs, cx) in enumerate(r64["hyps"]):
            assert r["beam_ids"][b][j].tolist() == toks, (what, k, b, j)
            worst = max(worst, abs(r["beam_score"][b][j] - s), abs(r["beam_ctc_score"][b][j] - cs), abs(r["beam_ctx_score"][b][j] - cx))
        print(f"{what} caller {k} utterance {b}: device error {worst:.3e}  bound {4 * e:.3e}")
        assert worst <= 4 * e
        off += n


def test_the_switch_is_accepted_and_off_by_default(pkg, model):
    assert model._lib.pfhip_svs_set_beam_merging(model._h, 1) == 0 and model._lib.pfhip_svs_set_beam_merging(model._h, 0) == 0
    assert model._lib.pfhip_svs_set_beam_merging(None, 1) == 1


def test_six_callers_share_forwards(model, audio, graphs, alone):
    assert int(alone[2]["frame_len"][0]) == 0 and alone[2]["beam_n_hyp"][0] == 0                   # the 0.02 s utterance: no rows
    # the lone calls themselves, on their own columns (read in this thread, right behind each)
    for k in BEAM:
        r = call(model, audio, graphs, k)
        cols = own_columns(model, r)
        assert cols is not None and cols[0] == max(s[0] for s in CALLERS[k][5])
        check_hypotheses(model, k, r, cols, graphs[k][1], "lone")

    def work(k):
        r = call(model, audio, graphs, k)
        return r, own_columns(model, r) if k in BEAM else None, model.debug_poke("svs_forward_calls")

    model.set_batching(WAIT_US, MAX_UTTS)
    model.set_beam_merging(True)
    f0, c0 = totals(model)
    try:
        got = in_threads(len(CALLERS), work)
    finally:
        model.set_beam_merging(False)
        model.set_batching(0, MAX_UTTS)
    f1, c1 = totals(model)
    worst = [0.0, 0.0]
    checked = 0
    for k, (r, cols, company) in enumerate(got):
        compare(r, alone[k], worst)
        if k not in BEAM:
            assert "beam_n_hyp" not in r
            continue
        assert r["beam_n_hyp"].tolist() == alone[k]["beam_n_hyp"].tolist()
        if cols is None:
            continue
        checked += 1
        check_hypotheses(model, k, r, cols, graphs[k][1], f"merged with {company - 1}")
    print(f"merged against lone: max |log-prob difference| {worst[0]:.3e}, max |score difference| {worst[1]:.3e} (bound {LOGP_TOL:.0e}); "
          f"{c1 - c0} calls in {f1 - f0} forwards; company {[g[2] for g in got]}; strides {[g[1][0] if g[1] else None for g in got]}; "
          f"{checked} of {len(BEAM)} beam callers still found their columns")
    assert worst[0] < LOGP_TOL and worst[1] < LOGP_TOL
    assert c1 - c0 == len(CALLERS) and f1 - f0 < c1 - c0
    assert any(got[k][2] > 1 for k in BEAM)             # a beam caller shared its forward
    assert checked >= 1


def test_switch_off_serves_every_beam_caller_alone(model, audio, graphs, alone):
    def work(i):
        r = call(model, audio, graphs, BEAM[i])
        return r, model.debug_poke("svs_forward_calls")

    model.set_batching(WAIT_US, MAX_UTTS)               # the queue is on, the switch is off: beam callers pass it by
    f0, c0 = totals(model)
    try:
        got = in_threads(len(BEAM), work)
    finally:
        model.set_batching(0, MAX_UTTS)
    f1, c1 = totals(model)
    assert c1 - c0 == len(BEAM) and f1 - f0 == len(BEAM) and all(g[1] == 1 for g in got)
    for i, k in enumerate(BEAM):                        # a forward of its own: the lone call's bits
        for b in range(len(alone[k]["ids"])):
            assert got[i][0]["frame_logp"][b].tobytes() == alone[k]["frame_logp"][b].tobytes()
            assert [x.tolist() for x in got[i][0]["beam_ids"][b]] == [x.tolist() for x in alone[k]["beam_ids"][b]]
            assert got[i][0]["beam_score"][b].tobytes() == alone[k]["beam_score"][b].tobytes()


def test_a_too_small_beam_buffer_fails_alone(pkg, model, audio, graphs, alone):
    ks = [4, 3, 0, 2]
    assert len(alone[3]["beam_ids"][0][0]) > 1

    def work(i):
        k = ks[i]
        if k == 3:
            with pytest.raises(pkg.PfhipError) as e:
                call(model, audio, graphs, k, beam_max_tokens=1)
            return e.value.status, e.value.beam_n_tokens
        return call(model, audio, graphs, k)

    model.set_batching(WAIT_US, MAX_UTTS)
    model.set_beam_merging(True)
    try:
        got = in_threads(len(ks), work)
    finally:
        model.set_beam_merging(False)
        model.set_batching(0, MAX_UTTS)
    status, n_tokens = got[1]
    assert status == 5                                  # PFHIP_ERR_CAPACITY, and the lengths it needs
    assert n_tokens.shape == (1, 2) and n_tokens[0].tolist() == [len(h) for h in alone[3]["beam_ids"][0]]
    worst = [0.0, 0.0]
    for i in (0, 2, 3):
        compare(got[i], alone[ks[i]], worst)
        if ks[i] in BEAM:
            assert got[i]["beam_n_hyp"].tolist() == alone[ks[i]]["beam_n_hyp"].tolist()
    assert worst[0] < LOGP_TOL and worst[1] < LOGP_TOL


def test_align_after_a_merged_beam_forward_is_the_callers_own(pkg, model, audio, graphs, alone):
    """align() on a merged caller's best hypotheses aligns against its own sub-range of the packed rows (or refuses because the
    context has run another forward since): the spans are those of the same align() behind its lone call; a score is a sum of one
    emission per speech row, each within LOGP_TOL of the lone forward's, so within rows x LOGP_TOL."""
    best = lambda r: [h[0] if len(h) else np.zeros(0, np.int32) for h in r["beam_ids"]]
    lone = {}
    for k in BEAM:
        r = call(model, audio, graphs, k)
        lone[k] = (r, model.align(best(r)))

    def work(k):
        r = call(model, audio, graphs, k)
        if k not in BEAM:
            return r, None
        try:
            return r, model.align(best(r))
        except pkg.PfhipError as e:
            assert e.status == 1 and "gone" in str(e), str(e)
            return r, None

    model.set_batching(WAIT_US, MAX_UTTS)
    model.set_beam_merging(True)
    try:
        got = in_threads(len(CALLERS), work)
    finally:
        model.set_beam_merging(False)
        model.set_batching(0, MAX_UTTS)
    served = 0
    for k in BEAM:
        r, al = got[k]
        if al is None or [x.tolist() for x in best(r)] != [x.tolist() for x in best(lone[k][0])]:
            continue
        served += 1
        for b in range(len(r["ids"])):
            assert al["begin"][b].tolist() == lone[k][1]["begin"][b].tolist() and al["end"][b].tolist() == lone[k][1]["end"][b].tolist()
            rows = max(int(r["frame_len"][b]) - 4, 0)
            if np.isfinite(lone[k][1]["score"][b]):
                assert abs(float(al["score"][b]) - float(lone[k][1]["score"][b])) <= rows * LOGP_TOL
    print(f"align after a merged beam forward: {served} of {len(BEAM)} beam callers still found their rows")
    assert served >= 1
