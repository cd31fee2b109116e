"""GPU: pfhip_svs_forward_spans — the SenseVoice forward with the spans of its own greedy tokens (ids[b][4:]) formed inside the forward
and returned in its one copy — on the three utterances of test_gpu_sensevoice_adapter.py (1.0 s, 0.02 s = no rows, 2.5 s).

No tolerance anywhere: what comes back beside the spans is pfhip_svs_forward's on the same input, and the spans are those of
pfhip_svs_align(ids[b][4:]) after that forward — the same rows through the same kernels, so any difference is a bug."""
import importlib

import numpy as np
import pytest

from conftest import synth_pcm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SECONDS = (1.0, 0.02, 2.5)
LIDS, TEXTNORMS = [4, 0, 3], [14, 15, 15]


@pytest.fixture(scope="module")
def model(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    wt = importlib.import_module("asr_2pass_amd.weights")
    m = pkg.SenseVoiceHip().InitAsr(wt.synth_svs_weights(), device=0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def utts():
    out = []
    for i, seconds in enumerate(SECONDS):
        x = synth_pcm(30 + i, int(seconds * 16000), np.random.default_rng(900 + i))
        out.append(np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_equal(got, plain, al):
    B = len(plain["ids"])
    assert got["token_num"].tolist() == plain["token_num"].tolist() and got["frame_len"].tolist() == plain["frame_len"].tolist()
    for b in range(B):
        for key in ("ids", "tok_frame", "tok_logp", "frame_ids", "frame_logp"):
            assert same_bits(got[key][b], plain[key][b]), (key, b)
        assert same_bits(got["span_begin"][b], al["begin"][b]), (b, got["span_begin"][b], al["begin"][b])
        assert same_bits(got["span_end"][b], al["end"][b]), (b, got["span_end"][b], al["end"][b])
        assert same_bits(got["span_logp"][b], al["logp"][b]), b
    assert same_bits(got["span_score"], al["score"]), (got["span_score"], al["score"])


def lone_pair(model, utts):
    plain = model.forward(utts, lid=LIDS, textnorm=TEXTNORMS)
    al = model.align([ids[4:] for ids in plain["ids"]])
    return plain, al


@pytest.mark.parametrize("s16", [True, False])
def test_spans_come_with_the_forward(model, utts, s16):
    din = utts if s16 else [u.astype(np.float32) / np.float32(32768.0) for u in utts]
    plain, al = lone_pair(model, din)
    got = model.forward(din, lid=LIDS, textnorm=TEXTNORMS, want_spans=True)
    check_equal(got, plain, al)
    # the case has something to show: tokens behind the tags on both utterances with rows, feasible paths, none for the one without
    assert len(al["begin"][0]) >= 1 and len(al["begin"][2]) > 4 and len(al["begin"][1]) == 0
    assert np.isfinite(al["score"][[0, 2]]).all() and al["score"][1] == 0.0
    assert (got["span_begin"][2] >= 4).all() and (got["span_end"][2] > got["span_begin"][2]).all()
    # and pfhip_svs_align still works behind a forward that brought its spans along: the same rows
    again = model.align([ids[4:] for ids in got["ids"]])
    check_equal(got, plain, again)


def test_spans_belong_to_the_range_guard_rerun(model, utts):
    """The range flag raised the way test_gpu_range_guard.py raises it: the forward is redone once on the exact kernels, and ids and
    spans are the re-run's — those of the plain forward and pfhip_svs_align under the same poke."""
    before = model.debug_poke("range_fallbacks")
    assert model.debug_poke("range_flag", 1) == 0
    plain, al = lone_pair(model, utts)
    assert model.debug_poke("range_fallbacks") == before + 1
    assert model.debug_poke("range_flag", 1) == 0
    got = model.forward(utts, lid=LIDS, textnorm=TEXTNORMS, want_spans=True)
    assert model.debug_poke("range_fallbacks") == before + 2
    check_equal(got, plain, al)
    assert len(al["begin"][2]) > 4 and np.isfinite(al["score"][2])


def test_an_utterance_beyond_the_capacity_is_refused_alone(model, utts):
    """"svs_span_cap" stands in for PFHIP_SVS_SPAN_MAX_FLOATS.  With room for the first utterance's emissions and not for the last
    one's, the last comes back as an infeasible one (spans -1, score -inf) and the others are served as ever."""
    plain, al = lone_pair(model, utts)
    n0, n2 = int(plain["frame_len"][0]) - 4, int(plain["frame_len"][2]) - 4
    l0, l2 = len(plain["ids"][0]) - 4, len(plain["ids"][2]) - 4
    cap = n0 * (l0 + 1) + n2 * (l2 + 1) - 1                # one float short of the last utterance's end
    assert cap < n0 * (n0 + 1) + n2 * (n2 + 1)             # below the host's own bound, so the poke is what limits
    try:
        assert model.debug_poke("svs_span_cap", cap) == 0
        got = model.forward(utts, lid=LIDS, textnorm=TEXTNORMS, want_spans=True)
        assert model.debug_poke("svs_span_cap", cap + 1) == 0
        fits = model.forward(utts, lid=LIDS, textnorm=TEXTNORMS, want_spans=True)
    finally:
        model.debug_poke("svs_span_cap", 0)
    check_equal(fits, plain, al)                            # one float more: everything fits
    for b in range(3):
        for key in ("ids", "tok_frame", "tok_logp", "frame_ids", "frame_logp"):
            assert same_bits(got[key][b], plain[key][b]), (key, b)
    for b in (0, 1):
        assert same_bits(got["span_begin"][b], al["begin"][b]) and same_bits(got["span_end"][b], al["end"][b])
        assert same_bits(got["span_logp"][b], al["logp"][b]) and same_bits(got["span_score"][b], al["score"][b])
    assert l2 > 0 and got["span_begin"][2].tolist() == [-1] * l2 and got["span_end"][2].tolist() == [-1] * l2
    assert np.isneginf(got["span_logp"][2]).all() and np.isneginf(got["span_score"][2])


def test_without_the_pointer_it_is_the_plain_forward(pkg, model, utts):
    """spans == NULL: pfhip_svs_forward_spans is pfhip_svs_forward; a too-small span buffer is PFHIP_ERR_CAPACITY."""
    import ctypes
    plain = model.forward(utts, lid=LIDS, textnorm=TEXTNORMS)
    B, cap = 3, max(int(n) for n in plain["frame_len"])
    ptrs = (ctypes.c_void_p * B)(*[u.ctypes.data for u in utts])
    ns = np.array([len(u) for u in utts], np.int32)
    lid, tn = np.array(LIDS, np.int32), np.array(TEXTNORMS, np.int32)
    ids, num = np.full((B, cap), -1, np.int32), np.zeros(B, np.int32)
    i32p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    out = pkg._SvsOut(ids.ctypes.data_as(i32p), num.ctypes.data_as(i32p), cap, None, None, None, None, None, None, 0)
    args = [model._h, ptrs, ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), B, lid.ctypes.data_as(i32p), tn.ctypes.data_as(i32p),
            ctypes.byref(out)]
    assert model._lib.pfhip_svs_forward_spans_s16(*args, None) == 0
    assert num.tolist() == plain["token_num"].tolist()
    for b in range(B):
        assert ids[b, :num[b]].tolist() == plain["ids"][b].tolist()
    begin, end = np.zeros((B, 2), np.int32), np.zeros((B, 2), np.int32)
    sp = pkg._SvsAlignOut(begin.ctypes.data_as(i32p), end.ctypes.data_as(i32p), None, None, 2)
    assert model._lib.pfhip_svs_forward_spans_s16(*args, ctypes.byref(sp)) == 5          # PFHIP_ERR_CAPACITY
