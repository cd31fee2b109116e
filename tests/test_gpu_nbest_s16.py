"""GPU: pfhip_offline_forward_nbest_s16, the candidates call on 16-bit PCM: bit for bit pfhip_offline_forward_nbest fed s / 32768.f
(ids, candidates, values), alone and with two callers merged by pfhip_set_batching."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FILL = -77


def tone_s16(rng, n, k=0):
    t = np.arange(n) / 16000.0
    x = 9000.0 * (0.6 * np.sin(2 * np.pi * (140.0 + 37.0 * k) * t) + 0.5 * rng.standard_normal(n))
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def ragged():
    """Three ragged utterances; the middle one is shorter than an fbank window (no token row) and holds both ends of the range."""
    rng = np.random.default_rng(31)
    utts = [tone_s16(rng, 16000 * 3 + 123, 0), tone_s16(rng, 200, 1), tone_s16(rng, 16000 * 2 + 7, 2)]
    utts[1][17], utts[1][18] = -32768, 32767
    return utts


def to_f32(u):
    return u.astype(np.float32) / np.float32(32768.0)


@pytest.fixture(scope="module")
def model(pkg, weights_mod):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=257)
    man, blob = weights_mod.synth_weights(cfg, seed=61)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    yield m
    m.close()


def same_result(a, b):
    for key in ("token_num", "n_fires", "n_frames"):
        assert np.array_equal(a[key], b[key]), key
    for x, y in zip(a["ids"], b["ids"]):
        assert np.array_equal(x, y)
    assert np.array_equal(a["nbest_ids"], b["nbest_ids"])
    assert np.array_equal(a["nbest_logp"].view(np.int32), b["nbest_logp"].view(np.int32))


def check_own(r, k):
    assert r["nbest_ids"].shape[2] == k
    for b in range(len(r["ids"])):
        nf, n = int(r["n_fires"][b]), len(r["ids"][b])
        assert np.array_equal(r["nbest_ids"][b, :n, 0], r["ids"][b])
        assert (np.diff(r["nbest_logp"][b, :nf], axis=1) <= 0).all()
        assert (r["nbest_ids"][b, nf:] == FILL).all()


def test_s16_equals_f32(model, pkg):
    utts = ragged()
    assert hasattr(pkg.load_lib(), "pfhip_offline_forward_nbest_s16")
    for k in (1, 5, 8):
        r16 = model.forward_ids(utts, nbest=k, nbest_fill=FILL, want_logp=True, nbest_s16=True)      # the s16 entry point
        r32 = model.forward_ids([to_f32(u) for u in utts], nbest=k, nbest_fill=FILL, want_logp=True)
        same_result(r16, r32)
        check_own(r16, k)
        for x, y in zip(r16["logp"], r32["logp"]):
            assert np.array_equal(x.view(np.int32), y.view(np.int32))
        assert int(r16["n_fires"][1]) == 0 and int(r16["n_fires"][0]) > 0 and int(r16["n_fires"][2]) > 0
    # the refusals of the f32 call
    with pytest.raises(pkg.PfhipError, match="status 1"):
        model.forward_ids(utts, nbest=9, nbest_s16=True)


def test_merged_callers(model):
    """pfhip_set_batching on, one execution slot, four s16 callers (k = 3, 5, 3, 5) arriving while a large batch holds the slot, so
    that they queue and are merged (the pattern of test_gpu_pcm16.test_mixed_formats_in_the_merge_queue).  Every caller sends the
    same utterance u, so a merged forward is j copies of u whatever the arrival order, and a caller's result must be, bit for bit,
    that of the unmerged F32 candidates call on [u / 32768.f] * j for some j (a forward of another composition may differ in the last
    bits); the values do not depend on the k a forward computes, so the references are computed with k = 5 and compared by prefix."""
    rng = np.random.default_rng(23)
    u16 = tone_s16(rng, 16000 + 333, 1)
    u32 = to_f32(u16)
    ks = (3, 5, 3, 5)
    want = [model.forward_ids([u32] * j, nbest=5, nbest_fill=FILL) for j in range(1, len(ks) + 1)]
    assert int(want[0]["n_fires"][0]) > 0
    blocker = [tone_s16(rng, 16000 * 20, k) for k in range(8)]       # 8 utterances = max_utterances: straight to the slot, not queued
    model.forward_ids(blocker)                                       # workspace sized before the merged calls
    model.set_batching(100000, 8)
    try:
        before = model.inflight_stats()
        got, err = [None] * len(ks), []
        gate = threading.Barrier(len(ks) + 1)

        def call(i):
            try:
                gate.wait()
                if i == len(ks):
                    model.forward_ids(blocker)
                else:
                    got[i] = model.forward_ids([u16], nbest=ks[i], nbest_fill=FILL, nbest_s16=True)
            except Exception as e:                                   # noqa: BLE001 (reported below)
                err.append(e)
        ths = [threading.Thread(target=call, args=(i,)) for i in range(len(ks) + 1)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert not err, err
        after = model.inflight_stats()
    finally:
        model.set_batching(0, 32)
    fw = sum(a["forwards"] - b["forwards"] for a, b in zip(after, before)) - 1          # without the blocker's
    assert fw < len(ks), (fw, "no two callers were merged")
    for g, k in zip(got, ks):
        check_own(g, k)
        n = int(g["n_fires"][0])
        assert any(int(w["n_fires"][0]) == n and np.array_equal(g["ids"][0], w["ids"][0])
                   and np.array_equal(g["nbest_ids"][0, :n], w["nbest_ids"][0, :n, :k])
                   and np.array_equal(g["nbest_logp"][0, :n].view(np.int32), w["nbest_logp"][0, :n, :k].view(np.int32)) for w in want)
