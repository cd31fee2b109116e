"""GPU: the SenseVoiceSmall offline forward (pfhip_svs_forward) on small_config_svs() — 512 / 4 heads of 128 / 2048, 2 + 2 layers,
vocabulary 1003, synthetic weights whose blank bias makes about half the frames blank and a quarter repeats — against the numpy
restatement tests/sensevoice_ref.py (float64 head).

Tolerances: frame ids follow conftest.assert_ids_match's rule (the runner-up is accepted where the float64 top-2 gap is below 1e-4)
for at most 0.5 % of the frames of a test; frame log-probs within 1e-3, the project's log-prob tolerance (check_against_oracle);
everything the collapse produces is compared EXACTLY with the Python collapse of the frame ids the device itself returned."""
import functools
import importlib

import numpy as np
import pytest

import sensevoice_ref as R
from conftest import synth_pcm
from oracle import paraformer as P

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LOGP_TOL = 1e-3
TIE_GAP = 1e-4
TIE_SHARE = 0.005
SECONDS = [0.02, 0.3, 1.0, 2.5, 5.0, 7.0]            # the first has 320 samples: no frame, no rows
LIDS = [0, 3, 4, 7, 11, 12]
TEXTNORMS = [14, 15, 14, 15, 15, 14]
PLANE_LIDS, PLANE_TEXTNORMS = [0, 3, 4, 7, 11, 12, 13, 0], [14, 15] * 4      # the 8 x 27 s pack


@functools.lru_cache(maxsize=None)
def container():
    wt = importlib.import_module("asr_2pass_amd.weights")
    man, blob = wt.synth_svs_weights()
    blob.setflags(write=False)
    return man, blob


@functools.lru_cache(maxsize=None)
def utterance(index, seconds):
    pcm = synth_pcm(index, int(round(seconds * 16000)), np.random.default_rng(4200 + index))
    pcm.setflags(write=False)
    return pcm


@functools.lru_cache(maxsize=None)
def reference(index, seconds, lid, textnorm):
    man, blob = container()
    return R.forward_pcm(utterance(index, seconds), P.Weights(man, blob), lid, textnorm)


@pytest.fixture(scope="module")
def model(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    m = pkg.SenseVoiceHip().InitAsr(container(), device=0)
    yield m
    m.close()


def check_utterance(got, b, ref, tally):
    """Utterance b of a forward against its reference; tally = [frames, frames on the tie rule]."""
    rows = ref["rows"]
    assert int(got["frame_len"][b]) == rows
    fid, flp = got["frame_ids"][b], got["frame_logp"][b]
    assert len(fid) == rows and len(flp) == rows
    for t in range(rows):
        if int(fid[t]) != int(ref["frame_ids"][t]):
            order = np.argsort(ref["logp"][t])
            gap = float(ref["logp"][t][order[-1]] - ref["logp"][t][order[-2]])
            assert gap < TIE_GAP and int(fid[t]) == int(order[-2]), f"utterance {b} frame {t}: got {fid[t]}, reference {ref['frame_ids'][t]} (gap {gap:.2e})"
            tally[1] += 1
    tally[0] += rows
    if rows:
        err = float(np.abs(flp - ref["logp"][np.arange(rows), fid]).max())
        assert err < LOGP_TOL, f"utterance {b}: frame log-prob max abs err {err}"
    # the collapse: exactly the Python collapse of the device's own frame ids
    ids, frames = R.ctc_collapse(fid, 0)
    assert int(got["token_num"][b]) == len(ids)
    assert got["ids"][b].tolist() == ids and got["tok_frame"][b].tolist() == frames
    want = flp[np.asarray(frames, np.int64)] if frames else np.zeros(0, np.float32)
    assert np.array_equal(got["tok_logp"][b].view(np.int32), want.view(np.int32))


def packed():
    return [utterance(i, s) for i, s in enumerate(SECONDS)]


def test_six_ragged_utterances(model):
    before = model.debug_poke("ctc_unfused_forwards")
    got = model.forward(packed(), lid=LIDS, textnorm=TEXTNORMS)
    tally = [0, 0]
    for b, s in enumerate(SECONDS):
        check_utterance(got, b, reference(b, s, LIDS[b], TEXTNORMS[b]), tally)
    assert tally[1] <= TIE_SHARE * tally[0], tally
    assert int(got["token_num"][0]) == 0 and int(got["frame_len"][0]) == 0          # 0.02 s: no rows, not even prompt rows
    assert sum(int(n) for n in got["token_num"]) > 20                                # the collapse had something to do ...
    # ... and something to drop.  The reference alone (numpy): 42 of these 284 frames are blank, 128 of the 242 others repeat their
    # predecessor (the frames of one utterance share most of their encoder row, so fewer are blank than on independent rows)
    blank = sum(int((f == 0).sum()) for f in got["frame_ids"])
    assert tally[0] == 284 and 20 < blank < 80 and sum(int(n) for n in got["token_num"]) < (284 - blank) - 60
    assert model.debug_poke("ctc_unfused_forwards") == before and model.debug_poke("range_fallbacks") == 0      # the fused head ran
    assert model.debug_poke("plane_forwards") == 0


def test_empty_batch_of_short_audio(model):
    got = model.forward([utterance(0, 0.02), utterance(0, 0.02)])
    assert got["token_num"].tolist() == [0, 0] and got["frame_len"].tolist() == [0, 0]


def test_batch_composition(model):
    """Each utterance alone equals its result in the pack (test_gpu_small_paraformer.py::test_batch_composition's assertion)."""
    together = model.forward(packed(), lid=LIDS, textnorm=TEXTNORMS)
    for b, u in enumerate(packed()):
        alone = model.forward([u], lid=[LIDS[b]], textnorm=[TEXTNORMS[b]])
        assert alone["frame_ids"][0].tolist() == together["frame_ids"][b].tolist()
        assert alone["ids"][0].tolist() == together["ids"][b].tolist()
        if len(alone["frame_logp"][0]):
            assert np.abs(alone["frame_logp"][0] - together["frame_logp"][b]).max() < 1e-4


def test_prompt_rows_are_attended_to(model):
    """lid and textnorm each change the rows after tp.norm."""
    u = [utterance(2, 1.0)]
    rows = model.rows_of(len(u[0]))
    encs = []
    for lid, tn in ((0, 15), (4, 15), (0, 14)):
        model.forward(u, lid=[lid], textnorm=[tn])
        encs.append(model.get_tensor("enc", rows * 512).reshape(rows, 512).copy())
    ref = reference(2, 1.0, 0, 15)
    e_enc = float(np.abs(encs[0] - ref["enc"]).max())
    print(f"SenseVoice: rows after tp.norm, max abs err {e_enc:.3e}")
    assert e_enc < 2e-4        # test_gpu_small_paraformer.py holds 3 layers + 1 LayerNorm to 1e-4; here 4 layers + 2 LayerNorms
    assert np.abs(encs[1] - encs[0])[4:].max() > 1e-3 and np.abs(encs[2] - encs[0])[4:].max() > 1e-3
    feats = model.get_tensor("feats", rows * 560).reshape(rows, 560)
    assert np.array_equal(feats[:4], R.prompt_rows(P.Weights(*container())["svs.embed.w"], 0, 14))      # the last forward: lid 0, textnorm 14
    assert np.abs(feats[4:] - ref["feats"][4:]).max() < 1e-3


def test_plane_path_crosses_the_hand_off(model):
    """8 x 27 s = 8 x 454 = 3632 rows, above the 3500-row switch to plane-image operands: enc.after_norm -> tp.0 is the one place
    where a layer with a residual has no producer's statistics or images to read."""
    utts = [utterance(10 + i, 27.0) for i in range(8)]
    lids, tns = PLANE_LIDS, PLANE_TEXTNORMS
    before = model.debug_poke("plane_forwards")
    got = model.forward(utts, lid=lids, textnorm=tns)
    assert model.debug_poke("plane_forwards") == before + 1
    assert model.debug_poke("range_fallbacks") == 0
    assert got["frame_len"].tolist() == [454] * 8
    tally = [0, 0]
    for b in range(8):            # ids / log-probs / collapse of every utterance, as in the ragged test
        check_utterance(got, b, reference(10 + b, 27.0, lids[b], tns[b]), tally)
    assert tally[0] == 3632 and tally[1] <= TIE_SHARE * tally[0], tally


def test_full_logp_rows_take_the_chunked_unfused_head(model):
    """Full rows requested: their arg-max is frame_ids, and the head ran over chunks of 2048 rows — 3632 rows are two chunks."""
    utts = [utterance(10 + i, 27.0) for i in range(8)]
    before = model.debug_poke("ctc_unfused_forwards")
    got = model.forward(utts, lid=PLANE_LIDS, textnorm=PLANE_TEXTNORMS, want_logp=True)
    assert model.debug_poke("ctc_unfused_forwards") == before + 1 and model.debug_poke("ctc_head_chunks") == 2
    for b in range(8):
        lp = got["logp"][b]
        assert lp.shape == (454, 1003)
        assert lp.argmax(axis=1).tolist() == got["frame_ids"][b].tolist()
        assert np.array_equal(lp[np.arange(454), got["frame_ids"][b]], got["frame_logp"][b])
        assert np.abs(np.log(np.exp(lp.astype(np.float64)).sum(axis=1))).max() < 1e-4          # rows are log-softmax rows
    for b in range(8):            # utterances 0-3 lie in the first chunk, 5-7 in the second, 4 across the cut
        assert np.abs(got["logp"][b] - reference(10 + b, 27.0, PLANE_LIDS[b], PLANE_TEXTNORMS[b])["logp"]).max() < LOGP_TOL


def test_unfused_head_by_debug_switch_agrees_with_the_fused_one(model):
    fused = model.forward(packed(), lid=LIDS, textnorm=TEXTNORMS)
    before = model.debug_poke("ctc_unfused_forwards")
    assert model.debug_poke("ctc_unfused", 1) == 0
    unfused = model.forward(packed(), lid=LIDS, textnorm=TEXTNORMS)
    assert model.debug_poke("ctc_unfused_forwards") == before + 1
    again = model.forward(packed(), lid=LIDS, textnorm=TEXTNORMS)
    assert model.debug_poke("ctc_unfused_forwards") == before + 1            # the switch holds for one forward
    for b in range(len(SECONDS)):
        assert unfused["frame_ids"][b].tolist() == fused["frame_ids"][b].tolist() == again["frame_ids"][b].tolist()
        if len(fused["frame_logp"][b]):
            assert np.abs(unfused["frame_logp"][b] - fused["frame_logp"][b]).max() < 1e-5


def test_range_guard_reruns_on_the_exact_kernels(model):
    """pfhip_debug_poke "range_flag": the forward finds its flag raised and is redone once on the exact kernels — bf16 GEMMs, the
    unfused chunked head — with results that meet the same reference."""
    before, unfused = model.debug_poke("range_fallbacks"), model.debug_poke("ctc_unfused_forwards")
    assert model.debug_poke("range_flag", 1) == 0
    got = model.forward(packed(), lid=LIDS, textnorm=TEXTNORMS)
    assert model.debug_poke("range_fallbacks") == before + 1 and model.debug_poke("ctc_unfused_forwards") == unfused + 1
    tally = [0, 0]
    for b, s in enumerate(SECONDS):
        check_utterance(got, b, reference(b, s, LIDS[b], TEXTNORMS[b]), tally)
    assert tally[1] <= TIE_SHARE * tally[0], tally
    model.forward(packed(), lid=LIDS, textnorm=TEXTNORMS)
    assert model.debug_poke("range_fallbacks") == before + 1                  # one forward only


def test_arguments_are_checked_before_any_launch(model, pkg):
    u = [utterance(2, 1.0)]
    for lid, tn in ((16, 15), (-1, 15), (0, 16)):
        with pytest.raises(pkg.PfhipError) as e:
            model.forward(u, lid=[lid], textnorm=[tn])
        assert e.value.status == 1                                            # PFHIP_ERR_ARG
    assert pkg.svs_lid("yue") == 7 and pkg.svs_lid("xx") == 0 and pkg.svs_lid(None) == 0 and pkg.svs_lid("nospeech") == 13


def test_kinds_refuse_each_other(model, pkg, weights_mod):
    """Every Paraformer entry point on a SenseVoice handle, and the SenseVoice call on a Paraformer handle: PFHIP_ERR_UNSUPPORTED."""
    import ctypes
    lib = model._lib
    assert lib.pfhip_is_ctc(model._h) == 1
    assert lib.pfhip_set_batching(model._h, 100, 8) == 4
    stream = ctypes.c_void_p()
    assert lib.pfhip_stream_create(model._h, None, ctypes.byref(stream)) == 4
    pf = pkg.ParaformerHip()
    pf._h = model._h                                                         # the Paraformer mirror's calls on this handle
    try:
        with pytest.raises(pkg.PfhipError) as e:
            pf.forward_ids([utterance(2, 1.0)])
        assert e.value.status == 4 and "pfhip_svs_forward" in str(e.value)
    finally:
        pf._h = ctypes.c_void_p()
    cfg = weights_mod.small_config(enc_layers=1, dec_layers=1)
    para = pkg.ParaformerHip().InitAsr(weights_mod.synth_weights(cfg), device=0)
    try:
        assert lib.pfhip_is_ctc(para._h) == 0
        sv = pkg.SenseVoiceHip()
        sv._h, sv.cfg = para._h, cfg
        try:
            with pytest.raises(pkg.PfhipError) as e:
                sv.forward([utterance(2, 1.0)])
            assert e.value.status == 4 and "pfhip_offline_forward" in str(e.value)
        finally:
            sv._h = ctypes.c_void_p()
    finally:
        para.close()


def test_capacity(model, pkg):
    """max_tokens below the longest kept sequence: PFHIP_ERR_CAPACITY; the counts are still filled."""
    import ctypes
    u = utterance(4, 5.0)
    i32p = ctypes.POINTER(ctypes.c_int32)
    ids, num = np.zeros(2, np.int32), np.zeros(1, np.int32)
    out = pkg._SvsOut()
    out.ids, out.token_num, out.max_tokens = ids.ctypes.data_as(i32p), num.ctypes.data_as(i32p), 2
    ptrs = (ctypes.c_void_p * 1)(u.ctypes.data)
    ns, lid, tn = np.array([len(u)], np.int32), np.array([0], np.int32), np.array([15], np.int32)
    st = model._lib.pfhip_svs_forward(model._h, ptrs, ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1, lid.ctypes.data_as(i32p),
                                      tn.ctypes.data_as(i32p), ctypes.byref(out))
    assert st == 5 and int(num[0]) > 2


def test_contexts_and_warm_up(model):
    """SenseVoice forwards go through the same execution contexts and warm-up as every other model."""
    model.set_inflight(2)
    try:
        model.warm_up(2, 16000)
        a = model.forward(packed(), lid=LIDS, textnorm=TEXTNORMS)
        b = model.forward(packed(), lid=LIDS, textnorm=TEXTNORMS)
        for x, y in zip(a["frame_ids"], b["frame_ids"]):
            assert x.tolist() == y.tolist()
    finally:
        model.set_inflight(1)
