"""CPU: the 16-bit PCM entry points of the C ABI (include/pfhip.h "16-bit PCM in") without a device: every *_s16 symbol is
exported, null and bad-argument calls come back PFHIP_ERR_ARG before any HIP call, and the Python wrappers route np.int16 audio
to the *_s16 symbols and float32 audio to the f32 ones (checked on a recording stand-in for the library: no compute)."""
import ctypes

import numpy as np
import pytest

S16_SYMBOLS = [
    "pfhip_offline_forward_s16", "pfhip_offline_forward_hwsets_s16", "pfhip_offline_forward_rate_s16", "pfhip_offline_enqueue_s16",
    "pfhip_offline_forward_resident_s16", "pfhip_vad_forward_sil_s16", "pfhip_stream_forward_s16", "pfhip_stream_forward_batch_s16",
    "pfhip_vad_stream_infer_s16", "pfhip_vad_stream_infer_batch_s16",
]
ERR_ARG = 1


@pytest.fixture(scope="module")
def lib(pkg):
    import os
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg.load_lib()


def test_every_s16_symbol_is_exported_and_bound(pkg, lib):
    for name in S16_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg.ABI_SYMBOLS, name
        assert getattr(lib, name).argtypes == getattr(lib, name[:-4]).argtypes, name        # the sibling's argument list


def test_null_and_bad_arguments_are_refused_without_a_device(pkg, lib):
    out = pkg._Out()
    n1 = (ctypes.c_int * 1)(16000)
    off = (ctypes.c_int64 * 1)(0)
    p1 = (ctypes.c_void_p * 1)(None)
    buf = np.zeros(16000, np.int16)
    pb = (ctypes.c_void_p * 1)(buf.ctypes.data)
    got = ctypes.c_int(0)
    sz = (ctypes.c_size_t * 1)(8)
    calls = {
        "pfhip_offline_forward_s16": lambda: lib.pfhip_offline_forward_s16(None, pb, n1, 1, None, 0, ctypes.byref(out)),
        "pfhip_offline_forward_hwsets_s16": lambda: lib.pfhip_offline_forward_hwsets_s16(None, pb, n1, 1, None, None, 0, None, ctypes.byref(out)),
        "pfhip_offline_forward_rate_s16": lambda: lib.pfhip_offline_forward_rate_s16(None, pb, n1, 1, 8000, None, 0, ctypes.byref(out)),
        "pfhip_offline_enqueue_s16": lambda: lib.pfhip_offline_enqueue_s16(None, buf.ctypes.data, off, n1, 1, None),
        "pfhip_offline_forward_resident_s16": lambda: lib.pfhip_offline_forward_resident_s16(None, buf.ctypes.data, off, n1, 1, ctypes.byref(out)),
        "pfhip_vad_forward_sil_s16": lambda: lib.pfhip_vad_forward_sil_s16(None, buf.ctypes.data, 16000, 1, None, 0, ctypes.byref(got)),
        "pfhip_stream_forward_s16": lambda: lib.pfhip_stream_forward_s16(None, buf.ctypes.data, 9600, 0, None, 0, ctypes.byref(got)),
        "pfhip_stream_forward_batch_s16": lambda: lib.pfhip_stream_forward_batch_s16(None, 1, pb, n1, n1, p1, n1, n1),
        "pfhip_vad_stream_infer_s16": lambda: lib.pfhip_vad_stream_infer_s16(None, buf.ctypes.data, 9600, 0, None, 0, ctypes.byref(got), None, 0,
                                                                             ctypes.byref(got)),
        "pfhip_vad_stream_infer_batch_s16": lambda: lib.pfhip_vad_stream_infer_batch_s16(None, 1, pb, n1, n1, p1, sz, n1, p1, sz, n1),
    }
    assert sorted(calls) == sorted(S16_SYMBOLS)
    for name, call in calls.items():
        assert call() == ERR_ARG, name
        assert lib.pfhip_last_error() not in (None, b""), name
    # a batch whose stream array holds a null, an empty batch
    assert lib.pfhip_stream_forward_batch_s16(p1, 1, pb, n1, n1, p1, n1, n1) == ERR_ARG
    assert lib.pfhip_stream_forward_batch_s16(p1, 0, pb, n1, n1, p1, n1, n1) == ERR_ARG
    assert lib.pfhip_vad_stream_infer_batch_s16(p1, 1, pb, n1, n1, p1, sz, n1, p1, sz, n1) == ERR_ARG
    assert lib.pfhip_vad_stream_infer_batch_s16(p1, 0, pb, n1, n1, p1, sz, n1, p1, sz, n1) == ERR_ARG


class RecordingLib:
    """Stands in for libpfhip.so: every function returns 0 (PFHIP_OK) and its name is logged."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("pfhip_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append(name)
            return {"pfhip_sample_rate": 16000, "pfhip_vocab_size": 8, "pfhip_vad_num_classes": 2}.get(name, 0)
        return fn

    def made(self):
        """The forward / infer calls since the last look."""
        got = [c for c in self.calls if "forward" in c or "infer" in c or "enqueue" in c]
        self.calls.clear()
        return got


def bare(cls, rec):
    obj = cls.__new__(cls)
    obj._lib = rec
    obj._h = ctypes.c_void_p(1)
    return obj


def test_python_wrappers_dispatch_on_dtype(pkg):
    rec = RecordingLib()
    s16 = [np.arange(1600, dtype=np.int16), np.arange(800, dtype=np.int16)]
    f32 = [x.astype(np.float32) / np.float32(32768.0) for x in s16]
    asr = bare(pkg.ParaformerHip, rec)
    asr._vocab = None
    hw = [np.zeros((2, 4), np.float32)]
    for din, sfx in ((s16, "_s16"), (f32, "")):
        asr.forward_ids(din)
        assert rec.made() == ["pfhip_offline_forward" + sfx]
        asr.forward_ids(din, sample_rate=8000)
        assert rec.made() == ["pfhip_offline_forward_rate" + sfx]
        asr.forward_ids(din, hw_sets=hw, set_of_utt=[0, 0])
        assert rec.made() == ["pfhip_offline_forward_hwsets" + sfx]
        asr.forward_ids(din, nbest=2)                                  # the candidates call takes floats only
        assert rec.made() == ["pfhip_offline_forward_nbest"]
    asr.forward_ids([s16[0], f32[1]])                                  # a mixed batch is one float batch
    assert rec.made() == ["pfhip_offline_forward"]
    off, ns = np.array([0, 1601]), np.array([1600, 800])
    for flag, sfx in ((True, "_s16"), (False, "")):
        asr.enqueue_device(4096, off, ns, s16=flag)
        assert rec.made() == ["pfhip_offline_enqueue" + sfx]
        asr.forward_resident(4096, off, ns, 8, s16=flag)
        assert rec.made() == ["pfhip_offline_forward_resident" + sfx]
    stream = bare(pkg.ParaformerOnlineHip, rec)
    vad = bare(pkg.FsmnVadHip, rec)
    vstream = bare(pkg.FsmnVadOnlineHip, rec)
    for din, sfx in ((s16, "_s16"), (f32, "")):
        stream.Forward(din[0])
        assert rec.made() == ["pfhip_stream_forward" + sfx]
        pkg.ParaformerOnlineHip.forward_batch([stream, stream], din, [False, False])
        assert rec.made() == ["pfhip_stream_forward_batch" + sfx]
        vad.ForwardSil(din[0])
        assert rec.made() == ["pfhip_vad_forward_sil" + sfx]
        vstream.InferScores(din[0])
        assert rec.made() == ["pfhip_vad_stream_infer" + sfx]
        pkg.FsmnVadOnlineHip.InferScoresBatch([vstream, vstream], din, [False, False])
        assert rec.made() == ["pfhip_vad_stream_infer_batch" + sfx]
    # entry points without an s16 form get s / 32768, never the raw integers
    assert np.array_equal(pkg._pcm_f32(s16[0]), f32[0])
    for obj in (asr, stream, vad, vstream):
        obj._h = ctypes.c_void_p()                                     # nothing to destroy
