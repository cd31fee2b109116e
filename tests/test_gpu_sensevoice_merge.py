"""GPU: concurrent SenseVoice callers merged into packed forwards (SenseVoiceHip.set_batching = pfhip_svs_set_batching, the sibling
of pfhip_set_batching for a CTC handle; pfhip_set_batching itself keeps refusing such a handle, as test_gpu_sensevoice.py pins).

Eight threads, released together, each with its own one or two utterances, its own language and ITN flag, either sample format.  What
a caller gets from a merged forward is compared with what the same call gave alone beforehand: ids, tok_frame, frame_ids and the
spans exactly; frame_logp, tok_logp and the scores within LOGP_TOL = 1e-4, the bound tests/test_gpu_forward.py::
test_batch_composition_invariance holds merged against lone forwards to (a packed row meets other neighbours in a GEMM tile; all row
counts here are far below the plane-path and large-grid thresholds, so lone and merged forwards run the same kernel family)."""
import importlib
import threading

import numpy as np
import pytest

from conftest import synth_pcm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LOGP_TOL = 1e-4
# per caller: seconds of its utterances, language, ITN, 16-bit samples
CALLERS = [((0.3, 1.1), "zh", True, True), ((2.5,), "en", False, False), ((0.02, 0.9), "auto", True, True), ((1.6,), "ja", False, True),
           ((0.7, 2.1), "ko", True, False), ((0.5,), "yue", False, False), ((1.3, 0.4), "en", True, True), ((1.9,), "zh", False, False)]
WAIT_US, MAX_UTTS = 200000, 8


@pytest.fixture(scope="module")
def model(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    wt = importlib.import_module("asr_2pass_amd.weights")
    m = pkg.SenseVoiceHip().InitAsr(wt.synth_svs_weights(), device=0)
    m.set_inflight(2)
    yield m
    m.close()


@pytest.fixture(scope="module")
def audio():
    out = []
    for k, (seconds, _, _, s16) in enumerate(CALLERS):
        utts = []
        for i, sec in enumerate(seconds):
            x = synth_pcm(10 * k + i, int(round(sec * 16000)), np.random.default_rng(7000 + 10 * k + i))
            utts.append(np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16) if s16 else x.astype(np.float32))
        out.append(utts)
    return out


@pytest.fixture(scope="module")
def alone(model, audio):
    """Every caller's call made alone, merging off: computed once, shared, left unchanged."""
    model.set_batching(0, MAX_UTTS)
    return [model.forward(audio[k], lang=c[1], itn=c[2], want_spans=True) for k, c in enumerate(CALLERS)]


def in_threads(n, work):
    """work(k) on n threads released by one barrier; returns the results, re-raises the first exception."""
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
        if "span_begin" in ref and "span_begin" in got:
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


def test_set_batching_is_accepted_on_a_ctc_handle(model):
    assert model._lib.pfhip_is_ctc(model._h) == 1
    model.set_batching(WAIT_US, MAX_UTTS)                                                          # raises unless PFHIP_OK
    assert model._lib.pfhip_svs_set_batching(model._h, WAIT_US, MAX_UTTS) == 0
    assert model._lib.pfhip_svs_set_batching(model._h, -1, MAX_UTTS) == 1 and model._lib.pfhip_svs_set_batching(model._h, 0, MAX_UTTS) == 0


def test_eight_callers_get_what_they_get_alone(model, audio, alone):
    assert any(len(r["span_begin"][b]) > 3 for r in alone for b in range(len(r["ids"])))          # there are spans to compare
    assert int(alone[2]["frame_len"][0]) == 0                                                      # the 0.02 s utterance: no rows
    model.set_batching(WAIT_US, MAX_UTTS)
    f0, c0 = totals(model)
    try:
        got = in_threads(len(CALLERS), lambda k: model.forward(audio[k], lang=CALLERS[k][1], itn=CALLERS[k][2], want_spans=True))
    finally:
        model.set_batching(0, MAX_UTTS)
    f1, c1 = totals(model)
    worst = [0.0, 0.0]
    for k in range(len(CALLERS)):
        compare(got[k], alone[k], worst)
    print(f"merged against lone: max |log-prob difference| {worst[0]:.3e}, max |score difference| {worst[1]:.3e} (bound {LOGP_TOL:.0e}); "
          f"{c1 - c0} calls in {f1 - f0} forwards")
    assert worst[0] < LOGP_TOL and worst[1] < LOGP_TOL
    assert c1 - c0 == len(CALLERS) and f1 - f0 < c1 - c0


def test_one_caller_wants_log_prob_rows(model, audio, alone):
    """Caller 1 asks for full rows among seven greedy callers and is made to SHARE a forward: it joins the queue only once the first
    of the others has come back (the lone first arrival, a few ms in), while the next leader is still inside its 200-ms gather window —
    which the utterance bound (32 here) cannot cut short.  Its rows are its lone call's within the bound, every row's arg-max is its
    frame id, and of that merged forward only ITS rows went through the unfused chunks: everybody served by the same forward reads
    rows_1, everybody else 0."""
    lone = model.forward(audio[1], lang=CALLERS[1][1], itn=CALLERS[1][2], want_logp=True)
    rows_1 = int(sum(alone[1]["frame_len"]))
    assert rows_1 > 20 and model.debug_poke("svs_unfused_rows") == rows_1 and model.debug_poke("svs_forward_calls") == 1
    model.forward(audio[1], lang=CALLERS[1][1], itn=CALLERS[1][2])
    assert model.debug_poke("svs_unfused_rows") == 0                                               # a greedy forward: the fused head alone
    ks = list(range(len(CALLERS)))
    first_back = threading.Event()

    def work(k):
        if k == 1:
            assert first_back.wait(timeout=60)
        r = model.forward(audio[k], lang=CALLERS[k][1], itn=CALLERS[k][2], want_logp=(k == 1))
        first_back.set()
        # of the forward that served this thread: the rows through the unfused chunks, the callers it served
        return r, model.debug_poke("svs_unfused_rows"), model.debug_poke("svs_forward_calls")

    model.set_batching(WAIT_US, 32)
    f0, c0 = totals(model)
    try:
        got = in_threads(len(ks), work)
    finally:
        model.set_batching(0, MAX_UTTS)
    f1, c1 = totals(model)
    assert c1 - c0 == len(ks) and f1 - f0 < len(ks)
    worst = [0.0, 0.0]
    for k in ks:
        compare(got[k][0], alone[k], worst)
    mine, unfused, company = got[1]
    print(f"the forward that served the log-prob caller served {company} callers; forwards {f1 - f0}, calls {c1 - c0}; "
          f"read-outs {[(g[1], g[2]) for g in got]}")
    assert company > 1                                                                             # it shared its forward ...
    assert unfused == rows_1                                                                       # ... of which only its rows were unfused
    assert all(g[1] in (0, rows_1) for g in got)
    assert sum(1 for g in got if g[1] == rows_1) == company and all(g[2] == company for g in got if g[1] == rows_1)
    err = float(np.abs(mine["logp"][0] - lone["logp"][0]).max())
    print(f"log-prob rows merged against lone: max abs difference {err:.3e}; other outputs {worst[0]:.3e} (bound {LOGP_TOL:.0e})")
    assert err < LOGP_TOL and worst[0] < LOGP_TOL
    assert np.argmax(mine["logp"][0], axis=1).tolist() == mine["frame_ids"][0].tolist()
    assert np.array_equal(mine["logp"][0][np.arange(rows_1), mine["frame_ids"][0]], mine["frame_logp"][0])


def test_a_too_small_buffer_fails_alone(pkg, model, audio, alone):
    ks = [4, 1, 7, 3]
    assert int(alone[1]["token_num"].max()) > 2

    def work(i):
        k = ks[i]
        if k == 1:
            with pytest.raises(pkg.PfhipError) as e:
                model.forward(audio[k], lang=CALLERS[k][1], itn=CALLERS[k][2], max_tokens=2)
            return e.value.status
        return model.forward(audio[k], lang=CALLERS[k][1], itn=CALLERS[k][2], want_spans=True)

    model.set_batching(WAIT_US, MAX_UTTS)
    try:
        got = in_threads(len(ks), work)
    finally:
        model.set_batching(0, MAX_UTTS)
    assert got[1] == 5                                                                             # PFHIP_ERR_CAPACITY
    worst = [0.0, 0.0]
    for i in (0, 2, 3):
        compare(got[i], alone[ks[i]], worst)
    assert worst[0] < LOGP_TOL and worst[1] < LOGP_TOL


def test_align_after_a_merged_forward_is_the_callers_own(pkg, model, audio, alone):
    """A caller's align() behind a merged forward aligns its own sub-range of the packed rows — the spans that came with the
    forward — or refuses because the context has run another forward since; never another caller's rows."""
    def work(k):
        r = model.forward(audio[k], lang=CALLERS[k][1], itn=CALLERS[k][2], want_spans=True)
        try:
            return r, model.align([ids[4:] for ids in r["ids"]])
        except pkg.PfhipError as e:
            assert e.status == 1 and "gone" in str(e), str(e)
            return r, None

    model.set_batching(WAIT_US, MAX_UTTS)
    try:
        got = in_threads(len(CALLERS), work)
    finally:
        model.set_batching(0, MAX_UTTS)
    served = 0
    for k, (r, al) in enumerate(got):
        compare(r, alone[k], [0.0, 0.0])
        if al is None:
            continue
        served += 1
        for b in range(len(r["ids"])):
            assert al["begin"][b].tolist() == r["span_begin"][b].tolist() and al["end"][b].tolist() == r["span_end"][b].tolist()
            assert al["logp"][b].tobytes() == r["span_logp"][b].tobytes()
        assert al["score"].tobytes() == r["span_score"].tobytes()
    print(f"align after a merged forward: {served} of {len(CALLERS)} callers still found their rows")
    assert served >= 1                                  # whoever was in the last forward of a context finds its rows
