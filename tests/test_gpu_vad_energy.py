"""GPU: the end-point detector's decibel track on the device and complete files scored in company.

  * the frame-energy kernel (pfhip_op_frame_energy[_s16]) is BITWISE the host loop: one float32 accumulator per frame, samples in
    ascending order, every product rounded to float32 before it is added.  The reference below is that loop in numpy float32
    arithmetic (no fusing, no widening) — oracle/e2e_vad.py's decibel track without the logarithm;
  * pfhip_vad_forward_sil_energy[_s16]: the energies of the call's own samples beside the unchanged silence posteriors;
  * pfhip_vad_forward_sil_batch[_s16]: several complete files in one pass — energies bitwise, posteriors within the VAD tolerance
    of tests/test_gpu_vad.py against the oracle (the GEMM kernel is picked from the packed row count), the handle's carried
    caches untouched;
  * pfhip_set_vad_batching: concurrent callers merged into such passes.

A workgroup of the kernel takes 64 frames, so 63 / 64 / 65 frames are the sizes around its only internal boundary."""
import threading

import numpy as np
import pytest

from conftest import synth_pcm
from oracle import fsmn_vad as V
from oracle import paraformer as P
from test_gpu_pipeline import shape_vad_weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TOL = 2e-5              # tests/test_gpu_vad.py's bound for the same quantity
WG_FRAMES = 64          # frames per workgroup (csrc/vad_energy.hip)


def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")


def n_frames(n, flen=400, fshift=160):
    return 0 if n < flen else 1 + (n - flen) // fshift


def energy_ref(w, flen=400, fshift=160):
    """The host loop: s = 0; for i in 0..flen-1: s += w[off + i] * w[off + i], in IEEE single."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    F = n_frames(w.size, flen, fshift)
    s = np.zeros(F, np.float32)
    idx = np.arange(F) * fshift
    for i in range(flen):
        x = w[idx + i]
        s += x * x
    return s


def to_f32(s16):
    return s16.astype(np.float32) / np.float32(32768.0)


def rand_s16(rng, n):
    return rng.integers(-32768, 32768, n).astype(np.int16)


@pytest.fixture(scope="module")
def ops(pkg):
    need_gpu()
    import importlib
    return importlib.import_module("asr_2pass_amd.ops")


def run_packed(ops, utts, offsets, dtype):
    """Packs the utterances at the given sample offsets into one device buffer (junk between them) and returns the per-utterance
    energies the kernel wrote."""
    total = max(o + len(u) for o, u in zip(offsets, utts)) + 3
    if dtype == np.int16:
        buf = np.full(total, 12345, np.int16)
    else:
        buf = np.full(total, 0.77, np.float32)
    for o, u in zip(offsets, utts):
        buf[o:o + len(u)] = u
    d = torch.from_numpy(buf).cuda()
    e, fo = ops.frame_energy(d, offsets, [len(u) for u in utts])
    e = e.cpu().numpy()
    return [e[fo[b]:fo[b + 1]] for b in range(len(utts))]


# ---- the operator ------------------------------------------------------------------------------------------------------------
EDGE_LENS = [399, 400, 559, 560] + [400 + 160 * (k - 1) for k in (WG_FRAMES - 1, WG_FRAMES, WG_FRAMES + 1)]


@pytest.mark.parametrize("n", EDGE_LENS)
def test_operator_edge_lengths(ops, n):
    """No frame, one frame, the last sample before / at the second frame, and one less than, exactly and one more than a
    workgroup's frames — each alone in its launch, f32 (squares need rounding) and s16."""
    rng = np.random.default_rng(n)
    x = (rng.random(n, dtype=np.float32) * 2 - 1).astype(np.float32)
    got, = run_packed(ops, [x], [0], np.float32)
    assert got.shape == (n_frames(n),)
    np.testing.assert_array_equal(got, energy_ref(x))
    s = rand_s16(rng, n)
    got, = run_packed(ops, [s], [0], np.int16)
    assert got.shape == (n_frames(n),)
    np.testing.assert_array_equal(got, energy_ref(to_f32(s)))


def test_operator_packed_batch_unaligned(ops):
    """Three utterances of unequal length, one of them empty: s16 utterances start at odd samples, f32 utterances at offsets that
    are no multiple of 4 floats; every 16-byte phase of the vector loads is taken, more than one workgroup per utterance."""
    rng = np.random.default_rng(7)
    for phase in range(8):
        lens = [400 + 160 * 70 + 37, 0, 400 + 160 * 3 + 159]
        o0 = 2 * phase + 1
        s_off = [o0, o0 + lens[0], o0 + lens[0] + 1]           # odd, (empty), odd: lens[0] is odd
        assert s_off[0] % 2 == 1 and s_off[2] % 2 == 1
        utts = [rand_s16(rng, n) for n in lens]
        got = run_packed(ops, utts, s_off, np.int16)
        for g, u in zip(got, utts):
            np.testing.assert_array_equal(g, energy_ref(to_f32(u)))
        assert got[1].size == 0 and got[0].size == 71 and got[2].size == 4
    for phase in (1, 2, 3):
        lens = [400 + 160 * 66 + 5, 0, 400 + 160 * 2]
        o2 = lens[0] + phase
        f_off = [phase, o2, o2 if o2 % 4 else o2 + 1]
        assert f_off[0] % 4 and f_off[2] % 4
        utts = [(rng.random(n, dtype=np.float32) * 2 - 1).astype(np.float32) for n in lens]
        got = run_packed(ops, utts, f_off, np.float32)
        for g, u in zip(got, utts):
            np.testing.assert_array_equal(g, energy_ref(u))


def test_operator_values(ops):
    """Full scale including -32768 (x = -1, e = 400 exactly), +-1 LSB (x^2 = 2^-30: sums far below one ulp of nothing), a frame
    of zeros (exactly 0), and full-scale random f32."""
    n = 400 + 160 * 5
    full = np.full(n, -32768, np.int16)
    full[1::2] = 32767
    lsb = np.ones(n, np.int16)
    lsb[::3] = -1
    zeros = np.zeros(n, np.int16)
    mixed = np.zeros(n, np.int16)
    mixed[560:] = -32768                                       # frame 0 all zeros, later frames partly / fully at full scale
    got = run_packed(ops, [full, lsb, zeros, mixed], [1, n + 3, 2 * n + 5, 3 * n + 7], np.int16)
    for g, u in zip(got, [full, lsb, zeros, mixed]):
        np.testing.assert_array_equal(g, energy_ref(to_f32(u)))
    assert np.all(got[2] == 0.0) and got[3][0] == 0.0 and got[3][-1] == 400.0
    assert np.all(got[1] == np.float32(400 * 2.0 ** -30))
    np.testing.assert_array_equal(run_packed(ops, [np.full(n, -32768, np.int16)], [0], np.int16)[0], np.full(6, 400.0, np.float32))
    # the f32 form fed s / 32768 is the s16 form
    np.testing.assert_array_equal(run_packed(ops, [to_f32(full)], [0], np.float32)[0], got[0])


def test_operator_other_window(ops):
    """flen / fshift are arguments: the 8 kHz detector's 200 / 80 (even shift: padded image) and an odd shift (image as it is)."""
    rng = np.random.default_rng(8)
    x = (rng.random(200 + 80 * 130 + 11, dtype=np.float32) * 2 - 1).astype(np.float32)
    for flen, fshift in ((200, 80), (75, 33)):
        d = torch.from_numpy(x).cuda()
        e, fo = ops.frame_energy(d, [0], [x.size], flen, fshift)
        np.testing.assert_array_equal(e.cpu().numpy(), energy_ref(x, flen, fshift))


# ---- the forward ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vad(pkg, weights_mod):
    need_gpu()
    man, blob = weights_mod.synth_vad_weights()
    h = pkg.FsmnVadHip().InitVad((man, blob))
    yield h, P.Weights(man, blob)
    h.close()


@pytest.fixture(scope="module")
def files(vad):
    """Five complete files (no samples, one short of a window, exactly one window, 3 s + 977, 12 s + 321) as s16, with the oracle's
    silence posteriors and the reference energies — computed once, shared, never modified."""
    _, W = vad
    rng = np.random.default_rng(31)
    out = []
    for i, n in enumerate((0, 399, 400, 16000 * 3 + 977, 16000 * 12 + 321)):
        s16 = np.clip(np.round(synth_pcm(i, n, rng) * 32768.0), -32768, 32767).astype(np.int16)
        f32 = to_f32(s16)
        sil = V.FsmnVad(W).Forward(f32, True)[:, 0] if n >= 400 else np.zeros(0, np.float32)
        for a in (s16, f32, sil):
            a.setflags(write=False)
        out.append({"s16": s16, "f32": f32, "sil": sil, "energy": energy_ref(f32)})
    return out


def test_forward_sil_energy(vad, files):
    h, _ = vad
    f = files[3]
    h.InitCache()
    sil0 = h.ForwardSil(f["f32"], is_final=True)
    sil, e = h.ForwardSilEnergy(f["f32"], is_final=True)
    np.testing.assert_array_equal(e, f["energy"])
    np.testing.assert_array_equal(sil, sil0)
    assert np.abs(sil - f["sil"]).max() < TOL
    sil16, e16 = h.ForwardSilEnergy(f["s16"], is_final=True)
    np.testing.assert_array_equal(sil16, sil)
    np.testing.assert_array_equal(e16, e)
    for k in (0, 1):                                           # no full window: no rows, no energies
        sil, e = h.ForwardSilEnergy(files[k]["s16"], is_final=True)
        assert sil.size == 0 and e.size == 0


def test_forward_sil_energy_slices(vad, files):
    """Slice-wise non-final calls: each returns the energies of ITS samples (frames that straddle two slices belong to neither,
    as in the reference's per-slice ComputeDecibel) and the scores of ForwardSil on the same sequence."""
    h, _ = vad
    pcm = files[3]["f32"]
    cuts = [0, 16000, 16400, 16799, 32000, len(pcm)]
    ref = []
    h.InitCache()
    for a, b in zip(cuts[:-1], cuts[1:]):
        ref.append(h.ForwardSil(pcm[a:b], is_final=b == len(pcm)))
    h.InitCache()
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        sil, e = h.ForwardSilEnergy(pcm[a:b], is_final=b == len(pcm))
        np.testing.assert_array_equal(sil, ref[k])
        np.testing.assert_array_equal(e, energy_ref(pcm[a:b]))
    h.InitCache()


def test_energy_capacity_error(pkg, vad, files):
    import ctypes
    h, _ = vad
    x = files[3]["f32"]
    cap = n_frames(x.size)
    sil, e = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
    n, ne = ctypes.c_int(0), ctypes.c_int(0)
    st = h._lib.pfhip_vad_forward_sil_energy(h._h, x.ctypes.data, int(x.size), 1, sil.ctypes.data, cap, ctypes.byref(n),
                                             e.ctypes.data, cap - 1, ctypes.byref(ne))
    assert st == 5 and ne.value == cap                         # PFHIP_ERR_CAPACITY, the count in *n_energy


@pytest.mark.parametrize("fmt", ["s16", "f32"])
def test_forward_sil_batch(vad, files, fmt):
    h, _ = vad
    got = h.ForwardSilBatch([f[fmt] for f in files])
    assert [len(s) for s, _ in got] == [0, 0, 1, 304, 1200] and [len(e) for _, e in got] == [0, 0, 1, 304, 1200]
    for (sil, e), f in zip(got, files):
        np.testing.assert_array_equal(e, f["energy"])
        if sil.size:
            assert np.abs(sil - f["sil"]).max() < TOL
    one = h.ForwardSilBatch([files[2][fmt]])                   # a pass of one file
    np.testing.assert_array_equal(one[0][1], files[2]["energy"])
    assert np.abs(one[0][0] - files[2]["sil"]).max() < TOL


def test_batch_leaves_carried_caches_alone(vad, files):
    """A packed pass issued in the middle of a slice-wise sequence: the sequence's carried caches are neither read nor written,
    so it still matches the oracle."""
    h, W = vad
    pcm = files[3]["f32"]
    o = V.FsmnVad(W)
    h.InitCache()
    cuts = [0, 16000, 32000, len(pcm)]
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        fin = b == len(pcm)
        ref = o.Forward(pcm[a:b], fin)[:, 0]
        sil, _ = h.ForwardSilEnergy(pcm[a:b], is_final=fin)
        assert np.abs(sil - ref).max() < TOL, k
        if k == 0:
            got = h.ForwardSilBatch([files[4]["s16"], files[3]["s16"]])
            assert np.abs(got[0][0] - files[4]["sil"]).max() < TOL and np.abs(got[1][0] - files[3]["sil"]).max() < TOL
    h.InitCache()


def test_batch_capacity_is_per_file(pkg, vad, files):
    import ctypes
    h, _ = vad
    xs = [files[2]["f32"], files[3]["f32"]]
    caps = [n_frames(x.size) for x in xs]
    sil = [np.zeros(c, np.float32) for c in caps]
    eng = [np.zeros(c, np.float32) for c in caps]
    ptr = lambda arrs: (ctypes.c_void_p * 2)(*[a.ctypes.data for a in arrs])
    ns = (ctypes.c_int * 2)(*[int(x.size) for x in xs])
    cs = (ctypes.c_size_t * 2)(*caps)
    ce = (ctypes.c_size_t * 2)(caps[0], caps[1] - 1)           # the second file's energy buffer is one short
    nf, ne = (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
    st = h._lib.pfhip_vad_forward_sil_batch(h._h, ptr(xs), ns, 2, ptr(sil), cs, nf, ptr(eng), ce, ne)
    assert st == 5 and list(nf) == caps and list(ne) == caps
    np.testing.assert_array_equal(eng[0], files[2]["energy"])  # the first file is served
    assert not eng[1].any() and not sil[1].any()               # the second got its counts and nothing else


def test_segments_from_energy_equal_segments_from_waveform(pkg, weights_mod):
    """sil + device energies through the energy detector == sil + waveform through the old one, on a file with real segments."""
    need_gpu()
    man, blob = shape_vad_weights(*weights_mod.synth_vad_weights())
    h = pkg.FsmnVadHip().InitVad((man, blob))
    rng = np.random.default_rng(41)
    parts = []
    for i, sec in enumerate((1.5, 2.2, 1.1)):
        parts += [synth_pcm(i, int(sec * 16000), rng), np.zeros(int(1.2 * 16000), np.float32)]
    pcm = np.concatenate(parts)
    sil, e = h.ForwardSilEnergy(pcm, is_final=True)
    n_used = 400 + 160 * (sil.size - 1)
    a, b = pkg.E2EVadModelHost(), pkg.E2EVadModelHost()
    want = a(sil, pcm[:n_used], True, False, 800, 60000, 0.9)
    got = b.feed_energy(sil, e[:sil.size], n_used, True, False, 800, 60000, 0.9)
    assert got == want and len(want) == 3
    a.close(); b.close(); h.close()


# ---- merging -----------------------------------------------------------------------------------------------------------------
def test_threads_are_merged(pkg, weights_mod):
    """Eight threads, one file each, with pfhip_set_vad_batching(2000, 8): energies bitwise those of lone calls, posteriors within
    TOL of the oracle, and at least one pass held more than one file.  With batching off the call is ForwardSilEnergy itself."""
    need_gpu()
    man, blob = weights_mod.synth_vad_weights()
    W = P.Weights(man, blob)
    h = pkg.FsmnVadHip().InitVad((man, blob))
    rng = np.random.default_rng(51)
    pcm = [np.clip(np.round(synth_pcm(i, 16000 * 2 + 531 * i, rng) * 32768.0), -32768, 32767).astype(np.int16) for i in range(8)]
    ref = [V.FsmnVad(W).Forward(to_f32(p), True)[:, 0] for p in pcm]
    alone = [h.ForwardSilEnergy(p, is_final=True) for p in pcm]
    assert h.batch_stats()["passes"] == 0                      # batching is off by default: lone calls, no packed pass
    for (sil, e), p, r in zip(alone, pcm, ref):
        np.testing.assert_array_equal(e, energy_ref(to_f32(p)))
        assert np.abs(sil - r).max() < TOL
    h.set_batching(2000, 8)
    merged = [None] * 8
    gate = threading.Barrier(8)

    def run(i):
        gate.wait()
        for _ in range(3):
            merged[i] = h.ForwardSilEnergy(pcm[i], is_final=True)

    th = [threading.Thread(target=run, args=(i,)) for i in range(8)]
    [t.start() for t in th]
    [t.join() for t in th]
    st = h.batch_stats()
    assert st["files"] == 24 and st["max_files"] > 1 and st["passes"] < 24, st
    for i in range(8):
        np.testing.assert_array_equal(merged[i][1], alone[i][1])
        assert merged[i][0].shape == ref[i].shape and np.abs(merged[i][0] - ref[i]).max() < TOL
    # a non-final call is never merged, and what follows it on the handle is not either (carried caches)
    before = h.batch_stats()["passes"]
    h.ForwardSilEnergy(pcm[0][:16000], is_final=False)
    h.ForwardSilEnergy(pcm[0][16000:], is_final=True)
    assert h.batch_stats()["passes"] == before
    h.InitCache()
    h.set_batching(0, 1)
    for i in (0, 5):
        sil, e = h.ForwardSilEnergy(pcm[i], is_final=True)
        np.testing.assert_array_equal(sil, alone[i][0])
        np.testing.assert_array_equal(e, alone[i][1])
    assert h.batch_stats()["passes"] == before
    h.close()
