"""GPU: the resampling kernel (csrc/resample.hip) and pfhip_offline_forward_rate.

The kernel must be bitwise equal to the NumPy restatement of the reference's LinearResample (tests/resample_ref.py) and to the
recordings of the reference's own resampler in tests/golden/resample_<fs>.npz (LinearResample from
onnxruntime/src/resample.cpp, compiled with -fPIC -g as its CMakeLists sets; -O2 gives the same bits, run as Audio::WavResample
runs it: cutoff 0.99*0.5*min(fs_in,16000), 6 zeros, flush=true, on seeded int16 inputs / 32768).
"""
import glob
import os

import numpy as np
import pytest
import torch

import resample_ref as R
from conftest import synth_pcm

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "resample_*.npz")))
RATES = [8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 96000, 7999, 16001]


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    import importlib
    return importlib.import_module("asr_2pass_amd.ops")


def _s16(rng, n):
    return (np.clip(np.round(8000 * rng.standard_normal(n)), -32768, 32767) / 32768.0).astype(np.float32)


def _run(ops, utts, fs_in, fs_out=16000, pad=3):
    """Packs utts with `pad` floats between them (unaligned starts), runs the kernel, returns the per-utterance outputs."""
    offs, o = [], 0
    for u in utts:
        offs.append(o)
        o += len(u) + pad
    host = np.full(max(o, 1), np.nan, np.float32)            # NaN between utterances: a read outside one would show
    for off, u in zip(offs, utts):
        host[off:off + len(u)] = u
    x = torch.from_numpy(host).cuda()
    y, out_off, n_out = ops.resample(x, offs, [len(u) for u in utts], fs_in, fs_out)
    torch.cuda.synchronize()
    yh = y.cpu().numpy()
    return [yh[a:a + n] for a, n in zip(out_off, n_out)]


@pytest.mark.parametrize("fs", RATES)
def test_kernel_bitwise_ragged_batch(ops, fs):
    rng = np.random.default_rng(fs)
    P, first, nt, w = R.cached_plan(fs, 16000)
    K = w.shape[1]
    span_in = int(np.ceil(1024 * fs / 16000))                  # input samples behind one 1024-output workgroup span
    lens = [0, 1, K - 1, K, K + 1, span_in - 1, span_in, span_in + 1, 2 * span_in + 1, fs * 30]
    lens += list(rng.integers(2, 3 * fs, 32 - len(lens)))
    utts = [_s16(rng, int(n)) for n in lens]
    got = _run(ops, utts, fs)
    for u, g in zip(utts, got):
        want = R.resample(u, fs)
        assert g.shape == want.shape, (fs, len(u))
        assert g.tobytes() == want.tobytes(), (fs, len(u), np.flatnonzero(g != want)[:5])


def test_kernel_aligned_and_batch_over_64(ops):
    rng = np.random.default_rng(5)
    utts = [_s16(rng, int(n)) for n in rng.integers(0, 20000, 70)]
    for g, u in zip(_run(ops, utts, 44100, pad=0), utts):
        assert g.tobytes() == R.resample(u, 44100).tobytes()


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_kernel_bitwise_equals_reference_recordings(ops, path):
    d = np.load(path)
    fs = int(d["fs_in"])
    utts = [d[f"in_{i}"].astype(np.float32) / np.float32(32768.0) for i in range(len(d["lengths"]))]
    for i, g in enumerate(_run(ops, utts, fs)):
        assert g.tobytes() == d[f"out_{i}"].tobytes(), (fs, i)


def test_other_output_rate(ops):
    rng = np.random.default_rng(9)
    utts = [_s16(rng, n) for n in (0, 5, 4000, 16000)]
    for fs_out in (8000, 44100):
        for g, u in zip(_run(ops, utts, 16000, fs_out), utts):
            assert g.tobytes() == R.resample(u, 16000, fs_out).tobytes()


@pytest.fixture(scope="module")
def plain(pkg, weights_mod):
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=300)
    man, blob = weights_mod.synth_weights(cfg, seed=41)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    yield m
    m.close()


def test_identity_is_a_copy(ops, plain):
    rng = np.random.default_rng(2)
    utts = [_s16(rng, n) for n in (0, 7, 16000)]
    utts[1][3] = -0.0
    for g, u in zip(_run(ops, utts, 16000), utts):
        assert g.tobytes() == u.tobytes()
    for g, u in zip(plain.resample(utts, 16000), utts):
        assert g.tobytes() == u.tobytes()


def test_handle_resample_matches_restatement_and_threads(pkg, plain):
    import threading
    rng = np.random.default_rng(3)
    utts = [_s16(rng, int(n)) for n in rng.integers(0, 48000 * 3, 6)]
    want = [R.resample(u, 48000) for u in utts]
    got = plain.resample(utts, 48000)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    errors = []

    def worker(k):
        try:
            for _ in range(3):
                fs = (8000, 44100, 48000, 12000)[k % 4]
                r = plain.resample(utts[:3], fs)
                if any(a.tobytes() != R.resample(u, fs).tobytes() for a, u in zip(r, utts[:3])):
                    errors.append(k)
        except Exception as e:                              # noqa: BLE001
            errors.append(repr(e))
    th = [threading.Thread(target=worker, args=(k,)) for k in range(16)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert errors == []


def test_unsupported_rates_refused(pkg, plain):
    for fs in (999, 192001, 160001):                        # out of range, out of range, lcm(160001, 16000) > int32
        with pytest.raises(pkg.PfhipError, match="status 4"):
            _raw_resample(pkg, plain, fs)
        with pytest.raises(pkg.PfhipError, match="status 4"):
            _raw_forward_rate(pkg, plain, fs)


def _raw_resample(pkg, m, fs):
    import ctypes
    x = np.zeros(100, np.float32)
    y = np.zeros(100, np.float32)
    ptrs = (ctypes.c_void_p * 1)(x.ctypes.data)
    optrs = (ctypes.c_void_p * 1)(y.ctypes.data)
    n = (ctypes.c_int * 1)(100)
    cap = (ctypes.c_int * 1)(100)
    got = (ctypes.c_int * 1)()
    pkg._check(m._lib, m._lib.pfhip_resample(m.handle, ptrs, n, 1, fs, optrs, cap, got))


def _raw_forward_rate(pkg, m, fs):
    import ctypes
    x = np.zeros(100, np.float32)
    ptrs = (ctypes.c_void_p * 1)(x.ctypes.data)
    n = (ctypes.c_int * 1)(100)
    out = pkg._Out()
    out.max_tokens = 4
    pkg._check(m._lib, m._lib.pfhip_offline_forward_rate(m.handle, ptrs, n, 1, fs, None, 0, ctypes.byref(out)))


def test_forward_rate_at_model_rate_is_forward(plain):
    rng = np.random.default_rng(4)
    utts = [synth_pcm(i, n, rng) for i, n in enumerate([16000 * 3, 16000 * 5 + 77, 300])]
    a = plain.forward_ids(utts, want_logp=True)
    b = plain.forward_ids(utts, want_logp=True, sample_rate=16000)
    for k in range(len(utts)):
        assert list(a["ids"][k]) == list(b["ids"][k])
        assert a["logp"][k].tobytes() == b["logp"][k].tobytes()


def _rate_audio(rng, fs, secs):
    return [_s16(rng, int(s * fs)) for s in secs]


@pytest.mark.parametrize("fs", [8000, 48000])
def test_forward_rate_equals_forward_of_resampled(plain, fs):
    rng = np.random.default_rng(fs + 1)
    utts = _rate_audio(rng, fs, [2.0, 3.3, 0.01, 4.7])
    a = plain.forward_ids(utts, want_logp=True, sample_rate=fs)
    b = plain.forward_ids([R.resample(u, fs) for u in utts], want_logp=True)
    for k in range(len(utts)):
        assert int(a["n_frames"][k]) == int(b["n_frames"][k])
        assert list(a["ids"][k]) == list(b["ids"][k])
        assert a["logp"][k].tobytes() == b["logp"][k].tobytes()


@pytest.mark.parametrize("fs", [8000, 48000])
def test_forward_rate_hotword_and_timestamp_models(pkg, weights_mod, fs):
    rng = np.random.default_rng(fs + 2)
    utts = _rate_audio(rng, fs, [2.5, 3.1])
    rs = [R.resample(u, fs) for u in utts]
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=2, vocab=400, contextual=1)
    m = pkg.ParaformerHip().InitAsr(weights_mod.synth_weights(cfg, seed=99))
    try:
        hw = m.CompileHotwordEmbedding([list(rng.integers(2, 400, n)) for n in (2, 3, 4)])
        a = m.forward_ids(utts, want_logp=True, hw_emb=hw, sample_rate=fs)
        b = m.forward_ids(rs, want_logp=True, hw_emb=hw)
        for k in range(len(utts)):
            assert list(a["ids"][k]) == list(b["ids"][k])
            assert a["logp"][k].tobytes() == b["logp"][k].tobytes()
    finally:
        m.close()
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=300, timestamp=1)
    m = pkg.ParaformerHip().InitAsr(weights_mod.synth_weights(cfg, seed=77))
    try:
        a = m.forward_ids(utts, want_logp=True, want_timestamps=True, sample_rate=fs)
        b = m.forward_ids(rs, want_logp=True, want_timestamps=True)
        for k in range(len(utts)):
            assert list(a["ids"][k]) == list(b["ids"][k])
            assert a["logp"][k].tobytes() == b["logp"][k].tobytes()
            assert a["us_alphas"][k].tobytes() == b["us_alphas"][k].tobytes()
            assert a["us_peaks"][k].tobytes() == b["us_peaks"][k].tobytes()
    finally:
        m.close()
