"""GPU: 16-bit PCM in (include/pfhip.h "16-bit PCM in").  An s16 sample s means the float s / 32768.f, and every *_s16 entry point
must give output BIT-IDENTICAL to its f32 sibling fed s.astype(float32) / 32768: the division and the front end's x 32768 are
exact powers of two, the fbank kernel's s16 form loads (float)s, the resampler's converts on load.  Every comparison below is
np.array_equal against the f32 sibling on the same handle — no tolerance anywhere."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LENS = [399, 400, 401, 1039, 16000]      # no frame, one frame, one frame + 1, odd, 1 s: packed offsets 0, 399, 799, 1200, 2239


def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")


def tone_s16(rng, n, k=0):
    t = np.arange(n) / 16000.0
    x = 9000.0 * (0.6 * np.sin(2 * np.pi * (140.0 + 37.0 * k) * t) + 0.5 * rng.standard_normal(n))
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def to_f32(u):
    return u.astype(np.float32) / np.float32(32768.0)


def ragged(seed=20):
    """The issue's batch: seeded random s16 of the lengths above; the 1039-sample utterance also holds both ends of the range."""
    rng = np.random.default_rng(seed)
    utts = [tone_s16(rng, n, k) for k, n in enumerate(LENS)]
    utts[3][17], utts[3][18], utts[3][400], utts[3][1038] = -32768, 32767, 32767, -32768
    return utts


def same_forward(a, b):
    for key in ("token_num", "n_fires", "n_frames"):
        assert np.array_equal(a[key], b[key]), key
    assert len(a["ids"]) == len(b["ids"])
    for x, y in zip(a["ids"], b["ids"]):
        assert np.array_equal(x, y)
    if a.get("logp") is not None or b.get("logp") is not None:
        for x, y in zip(a["logp"], b["logp"]):
            assert x.shape == y.shape and np.array_equal(x, y)
    for key in ("us_alphas", "us_peaks"):
        if key in a or key in b:
            for x, y in zip(a[key], b[key]):
                assert np.array_equal(x, y), key


@pytest.fixture(scope="module")
def plain(pkg, weights_mod):
    need_gpu()
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=257)
    man, blob = weights_mod.synth_weights(cfg, seed=61)
    model = pkg.ParaformerHip().InitAsr((man, blob))
    yield model, (man, blob)
    model.close()


@pytest.fixture(scope="module")
def stamped(pkg, weights_mod):
    """The same shape with the timestamp head (us_alphas / us_cif_peak outputs)."""
    need_gpu()
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=257, timestamp=1)
    man, blob = weights_mod.synth_weights(cfg, seed=62)
    model = pkg.ParaformerHip().InitAsr((man, blob))
    yield model, (man, blob)
    model.close()


def test_ragged_edges_host_buffers(plain):
    """pfhip_offline_forward_s16 on the ragged batch: the feature matrix (pfhip_get_tensor "feats"), log-probs, ids and token_num
    equal the f32 call's."""
    model, _ = plain
    utts = ragged()
    cap = 64 * 560
    got16 = model.forward_ids(utts, want_logp=True)
    feats16 = model.get_tensor("feats", cap).copy()
    got32 = model.forward_ids([to_f32(u) for u in utts], want_logp=True)
    feats32 = model.get_tensor("feats", cap).copy()
    assert list(got16["n_frames"]) == [0, 1, 1, 1, 17] and feats16.size == 20 * 560
    assert np.array_equal(feats16, feats32)
    same_forward(got16, got32)
    assert sum(int(n) for n in got16["n_fires"]) > 0


def test_timestamp_outputs(stamped):
    """us_alphas / us_cif_peak of a timestamp model through pfhip_offline_forward_s16."""
    model, _ = stamped
    rng = np.random.default_rng(22)
    utts = [tone_s16(rng, 16000 * 2 + 1, 1), tone_s16(rng, 16000 + 4801, 2)]
    got16 = model.forward_ids(utts, want_logp=True, want_timestamps=True)
    got32 = model.forward_ids([to_f32(u) for u in utts], want_logp=True, want_timestamps=True)
    assert min(a.size for a in got16["us_alphas"]) > 0
    same_forward(got16, got32)


def packed(utts):
    off = np.concatenate([[0], np.cumsum([len(u) for u in utts])[:-1]]).astype(np.int64)
    return off, np.array([len(u) for u in utts], np.int32), np.concatenate(utts)


def test_odd_alignment_resident_path(plain):
    """The same utterances back to back in ONE device s16 buffer (three of them start at odd samples: 2-byte alignment only)
    through pfhip_offline_enqueue_s16 + pfhip_offline_fetch, again with pfhip_set_nbest(3) + pfhip_offline_fetch_nbest, and through
    pfhip_offline_forward_resident_s16."""
    model, _ = plain
    off, ns, flat = packed(ragged())
    assert sum(int(o) & 1 for o in off) >= 2
    d16 = torch.from_numpy(flat).cuda()
    d32 = torch.from_numpy(to_f32(flat)).cuda()
    torch.cuda.synchronize()
    B, V = len(ns), 257

    def run(dev, s16, k):
        model.set_nbest(k)
        model.enqueue_device(dev.data_ptr(), off, ns, s16=s16)
        r = model.fetch(B, 32)
        if k:
            r["nb_ids"], r["nb_logp"] = model.fetch_nbest(B, 32, k, fill=-7)
        r["logp_rows"] = model.get_tensor("logp", 64 * V).copy()
        r["feats"] = model.get_tensor("feats", 64 * 560).copy()
        return r

    for k in (0, 3):
        a, b = run(d16, True, k), run(d32, False, k)
        same_forward(a, b)
        assert np.array_equal(a["feats"], b["feats"]) and a["feats"].size == 20 * 560
        assert a["logp_rows"].size > 0 and np.array_equal(a["logp_rows"], b["logp_rows"])
        if k:
            assert np.array_equal(a["nb_ids"], b["nb_ids"]) and np.array_equal(a["nb_logp"], b["nb_logp"])
            assert (a["nb_ids"] != -7).any()
    model.set_nbest(0)
    same_forward(model.forward_resident(d16.data_ptr(), off, ns, 32, s16=True), model.forward_resident(d32.data_ptr(), off, ns, 32))
    # and the resident results are those of the host-buffer form
    same_forward(model.forward_resident(d16.data_ptr(), off, ns, 32, s16=True), model.forward_ids(ragged(), max_tokens=32))


@pytest.mark.parametrize("fs,lens", [(8000, [4000, 4001, 150]), (44100, [22050, 22051, 1001])])
def test_resampling(plain, fs, lens):
    """pfhip_offline_forward_rate_s16: the resampler converts on load; about 0.5 s per utterance, one of odd length, one too short
    for a frame (and, packed, starting at a sample that is no multiple of 4 bytes' worth)."""
    model, _ = plain
    rng = np.random.default_rng(fs)
    utts = [tone_s16(rng, n, k) for k, n in enumerate(lens)]
    utts[1][5], utts[1][6] = -32768, 32767
    got16 = model.forward_ids(utts, want_logp=True, sample_rate=fs)
    feats16 = model.get_tensor("feats", 64 * 560).copy()
    got32 = model.forward_ids([to_f32(u) for u in utts], want_logp=True, sample_rate=fs)
    feats32 = model.get_tensor("feats", 64 * 560).copy()
    assert feats16.size > 0 and np.array_equal(feats16, feats32)
    same_forward(got16, got32)
    assert int(got16["n_frames"][0]) > 0 and int(got16["n_frames"][2]) == 0


def test_hotword_sets(pkg, weights_mod):
    """pfhip_offline_forward_hwsets_s16 on the contextual small-shape model of the hotword tests: two sets over three utterances."""
    need_gpu()
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=2, vocab=400, contextual=1)
    man, blob = weights_mod.synth_weights(cfg, seed=99)
    model = pkg.ParaformerHip().InitAsr((man, blob))
    rng = np.random.default_rng(32)
    sets = [model.CompileHotwordEmbedding([list(rng.integers(2, 400, int(rng.integers(1, 8)))) for _ in range(n)]) for n in (3, 6)]
    utts = [tone_s16(rng, n, k) for k, n in enumerate((16000 * 2 + 1, 16000 * 3, 16000 * 2 + 777))]
    got16 = model.forward_ids(utts, want_logp=True, hw_sets=sets, set_of_utt=[0, 1, 0])
    got32 = model.forward_ids([to_f32(u) for u in utts], want_logp=True, hw_sets=sets, set_of_utt=[0, 1, 0])
    same_forward(got16, got32)
    assert min(int(n) for n in got16["n_fires"]) > 0
    # one set for all (pfhip_offline_forward_s16 with hw_emb)
    same_forward(model.forward_ids(utts, want_logp=True, hw_emb=sets[1]), model.forward_ids([to_f32(u) for u in utts], want_logp=True, hw_emb=sets[1]))
    model.close()


def test_range_guard_rerun_remembers_the_format(plain):
    """A forward whose range flag is raised (pfhip_debug_poke "range_flag") is redone on the exact kernels from the saved PCM pointer:
    the re-run of an s16 enqueue must read shorts again, and equal the re-run of the f32 call."""
    model, _ = plain
    off, ns, flat = packed(ragged(21))
    d16 = torch.from_numpy(flat).cuda()
    d32 = torch.from_numpy(to_f32(flat)).cuda()
    torch.cuda.synchronize()
    res = []
    for dev, s16 in ((d16, True), (d32, False)):
        before = model.debug_poke("range_fallbacks")
        assert model.debug_poke("range_flag", 1) == 0
        model.enqueue_device(dev.data_ptr(), off, ns, s16=s16)
        r = model.fetch(len(ns), 32)
        assert model.debug_poke("range_fallbacks") == before + 1
        r["logp_rows"] = model.get_tensor("logp", 64 * 257).copy()
        r["feats"] = model.get_tensor("feats", 64 * 560).copy()
        res.append(r)
    same_forward(res[0], res[1])
    assert res[0]["logp_rows"].size > 0 and np.array_equal(res[0]["logp_rows"], res[1]["logp_rows"])
    assert np.array_equal(res[0]["feats"], res[1]["feats"])


def test_mixed_formats_in_the_merge_queue(pkg, plain):
    """pfhip_set_batching on, ONE execution slot, six threads calling at once with s16 and f32 (alternating) of the same audio while
    a large batch holds the slot: both formats queue together behind it, so the leader's pick has to split the queue by format
    (pfhip_debug_poke "format_splits" counts it) — a packed forward that mixed them would read shorts as floats.  The six calls are
    served by fewer forwards than calls (merged) and at least two (one per format).

    Every caller sends the same utterance u, so a merged forward is k copies of u in one format whatever the arrival order, and its
    per-utterance result is that of the unmerged call on [u] * k — the reference of the same batch composition, bit for bit (a
    forward of another composition may differ in the last bits: offline_api.cpp, "cross-request batching").  k is not observable per caller:
    each result must equal the reference of some k, the two formats' references are checked equal beforehand, and the lone two-thread
    case of the issue (k = 1: the unmerged call itself) is among them."""
    _, (man, blob) = plain
    model = pkg.ParaformerHip().InitAsr((man, blob))
    rng = np.random.default_rng(23)
    u16 = tone_s16(rng, 16000 + 333, 1)
    u32 = to_f32(u16)
    n_callers = 6
    want = []
    for k in range(1, n_callers // 2 + 1):          # unmerged calls (batching off): k copies of u
        w = model.forward_ids([u16] * k, want_logp=True)
        same_forward(w, model.forward_ids([u32] * k, want_logp=True))
        for b in range(1, k):                       # the copies of one batch agree among themselves
            assert np.array_equal(w["logp"][b], w["logp"][0]) and np.array_equal(w["ids"][b], w["ids"][0])
        want.append(w)
    assert int(want[0]["n_fires"][0]) > 0
    blocker = [tone_s16(rng, 16000 * 20, k) for k in range(8)]       # 8 utterances = max_utterances: straight to the slot, not queued
    model.forward_ids(blocker)                                       # workspace sized outside the timed part
    model.set_batching(100000, 8)
    for form in ("s16 first", "f32 first"):
        before, splits0 = model.inflight_stats(), model.debug_poke("format_splits")
        got, err = [None] * n_callers, [None] * (n_callers + 1)
        gate = threading.Barrier(n_callers + 1)

        def call(i):
            try:
                gate.wait()
                if i == n_callers:
                    model.forward_ids(blocker)
                else:
                    got[i] = model.forward_ids([u16 if (i % 2 == 0) == (form == "s16 first") else u32], want_logp=True)
            except Exception as e:       # noqa: BLE001 (reported below)
                err[i] = e
        ths = [threading.Thread(target=call, args=(i,)) for i in range(n_callers + 1)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert err == [None] * (n_callers + 1), err
        after = model.inflight_stats()
        fw = sum(a["forwards"] - b["forwards"] for a, b in zip(after, before)) - 1          # without the blocker's
        calls = sum(a["calls"] - b["calls"] for a, b in zip(after, before)) - 1
        assert calls == n_callers and 2 <= fw < calls, (fw, calls)                          # merged, and not into one forward
        assert model.debug_poke("format_splits") > splits0, "f32 and s16 callers never met in the queue"
        for g in got:
            assert int(g["n_fires"][0]) == int(want[0]["n_fires"][0]) and np.array_equal(g["ids"][0], want[0]["ids"][0])
            assert any(np.array_equal(g["logp"][0], w["logp"][0]) for w in want)
    model.close()


def test_streaming(pkg, weights_mod):
    """pfhip_stream_forward_s16: three 9600-sample chunks and a short final call; then a round of three connections through
    pfhip_stream_forward_batch_s16.  Ids and log-prob rows equal the f32 streams' call by call."""
    need_gpu()
    cfg = weights_mod.small_config(enc_layers=3, dec_layers=2, vocab=517)
    man, blob = weights_mod.synth_weights(cfg, seed=77)
    model = pkg.ParaformerHip().InitAsr((man, blob))
    rng = np.random.default_rng(24)
    pcm = tone_s16(rng, 9600 * 3 + 700, 3)
    a, b = pkg.ParaformerOnlineHip(model), pkg.ParaformerOnlineHip(model)
    a.set_debug(True); b.set_debug(True)
    pos, n_ids, n_rows = 0, 0, 0
    for n, fin in [(9600, False)] * 3 + [(700, True)]:
        seg = pcm[pos:pos + n]
        pos += n
        ids16 = a.Forward(seg, input_finished=fin)
        lp16 = a.get_tensor("logp", 128 * 517).copy()
        ids32 = b.Forward(to_f32(seg), input_finished=fin)
        lp32 = b.get_tensor("logp", 128 * 517).copy()
        assert ids16 == ids32 and a.last_path() == b.last_path()
        assert np.array_equal(lp16, lp32)
        n_ids += len(ids16); n_rows += lp16.size
    assert n_ids > 0 and n_rows > 0
    a.close(); b.close()
    s16 = [pkg.ParaformerOnlineHip(model) for _ in range(3)]
    s32 = [pkg.ParaformerOnlineHip(model) for _ in range(3)]
    for s in s16 + s32:
        s.set_debug(True)
    conn = [tone_s16(rng, n, k) for k, n in enumerate((9600 * 2, 9600 + 4801, 9600 * 2 - 1))]
    fired = 0
    for step in range(2):
        dins = [c[9600 * step:9600 * (step + 1)] for c in conn]
        fins = [step == 1] * 3
        got16 = pkg.ParaformerOnlineHip.forward_batch(s16, dins, fins)
        lp16 = [s.get_tensor("logp", 128 * 517).copy() for s in s16]
        got32 = pkg.ParaformerOnlineHip.forward_batch(s32, [to_f32(d) for d in dins], fins)
        lp32 = [s.get_tensor("logp", 128 * 517).copy() for s in s32]
        assert got16 == got32
        for x, y in zip(lp16, lp32):
            assert np.array_equal(x, y)
        fired += sum(len(g) for g in got16)
    assert fired > 0
    for s in s16 + s32:
        s.close()
    model.close()


def test_vad(pkg, weights_mod):
    """pfhip_vad_forward_sil_s16 on 1 s; pfhip_vad_stream_infer_s16 with two 600-ms feeds and a final one; one
    pfhip_vad_stream_infer_batch_s16 round.  Scores and the waveform handed to the end-point detector equal the f32 calls'."""
    need_gpu()
    man, blob = weights_mod.synth_vad_weights()
    vad = pkg.FsmnVadHip().InitVad((man, blob))
    rng = np.random.default_rng(25)
    pcm = tone_s16(rng, 16000, 4)
    pcm[100], pcm[101] = -32768, 32767
    vad.InitCache()
    sil16 = vad.ForwardSil(pcm, is_final=True)
    vad.InitCache()
    sil32 = vad.ForwardSil(to_f32(pcm), is_final=True)
    assert sil16.size == 98 and np.array_equal(sil16, sil32)
    a, b = pkg.FsmnVadOnlineHip(vad), pkg.FsmnVadOnlineHip(vad)
    long = tone_s16(rng, 9600 * 2 + 3001, 5)
    rows = 0
    for lo, hi, fin in ((0, 9600, False), (9600, 19200, False), (19200, len(long), True)):
        s16, w16 = a.InferScores(long[lo:hi], input_finished=fin)
        s32, w32 = b.InferScores(to_f32(long[lo:hi]), input_finished=fin)
        assert np.array_equal(s16, s32) and np.array_equal(w16, w32)
        rows += s16.size
    assert rows > 0
    a.close(); b.close()
    c16 = [pkg.FsmnVadOnlineHip(vad) for _ in range(3)]
    c32 = [pkg.FsmnVadOnlineHip(vad) for _ in range(3)]
    waves = [tone_s16(rng, n, k) for k, n in enumerate((9600, 9601, 4799))]
    got16 = pkg.FsmnVadOnlineHip.InferScoresBatch(c16, waves, [False, False, True])
    got32 = pkg.FsmnVadOnlineHip.InferScoresBatch(c32, [to_f32(w) for w in waves], [False, False, True])
    for (s_a, w_a), (s_b, w_b) in zip(got16, got32):
        assert np.array_equal(s_a, s_b) and np.array_equal(w_a, w_b)
    assert sum(s.size for s, _ in got16) > 0
    for c in c16 + c32:
        c.close()
    vad.close()


def test_handle_api_passes_the_callers_bytes(pkg, stamped, weights_mod, tmp_path):
    """FunOfflineInferBuffer (C++ mirror, `offline_infer` harness) on one short s16 buffer: the adapter hands the caller's bytes to
    ParaformerHip::ForwardPcm16; ids, text and stamps are those of the f32 C-ABI path assembled here (pfhip_offline_forward on
    s / 32768 -> TimestampOnnx -> the adapter's ms pairs; no vocabulary file: ids as text, stamps straight from the spans)."""
    model, (man, blob) = stamped
    rng = np.random.default_rng(26)
    s16 = tone_s16(rng, 16000 * 3 + 501, 6)
    mdir = tmp_path / "asr"
    mdir.mkdir()
    weights_mod.save(str(mdir / "model.pfhip"), man, blob)
    s16.astype("<i2").tofile(tmp_path / "short.pcm")
    exe = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "offline_infer")
    out = subprocess.run([exe, str(mdir), "-", str(tmp_path / "short.pcm"), "4", "1", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    want = model.forward_ids([to_f32(s16)], want_timestamps=True)
    ids = [int(i) for i in want["ids"][0]]
    assert len(ids) > 0
    seg = [l for l in lines if l.startswith("seg ")]
    assert len(seg) == 1
    head, _, tail = seg[0].partition(":")
    assert [int(x) for x in head.split()[1:3]] == [0, len(s16)] and [int(x) for x in tail.split()] == ids
    assert [l for l in lines if l.startswith("text ")][0][5:] == " ".join(str(i) for i in ids)
    n_chars = len(ids) - (1 if ids[-1] == 2 else 0)
    spans = pkg.timestamp_onnx(want["us_alphas"][0], want["us_peaks"][0], n_chars)
    pairs = [[int(np.float32(1000) * (np.float32(b) + np.float32(0))), int(np.float32(1000) * (np.float32(e) + np.float32(0)))]
             for b, e, sil in spans if not sil]
    stamp = [l for l in lines if l.startswith("stamp ")][0][6:]
    assert len(pairs) > 0 and json.loads(stamp) == pairs
