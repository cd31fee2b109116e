"""GPU: the kernels that start every request, each through its own operator entry (include/pfhip_ops.h): the fused fbank kernel in both
launch forms and both sample formats against an fp64 fbank, the LFR/CMVN family and the batched row copy against exact references, and
the positional-encoding kernels against fp64 sines of the fp32 argument.

The fbank cases, their fp64 references and the comparison are tests/frontend_ref.py's; tests/test_frontend_ref.py shows on the CPU that
the comparison fails, by 10 times its bound or more, for a kernel with any of eight seeded defects.  Conventions of
tests/test_gpu_row_ops.py: outputs start as a canary that is compared bit for bit outside the region written, every output element is
compared, every tolerance-based test prints error over bound before it asserts and carries the value measured on the MI355X.
"""
import importlib

import numpy as np
import pytest

import frontend_ref as R
from oracle import frontend as FE

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32, F64 = np.float32, np.float64
CANARY = F32(-1234.5)


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def canary(shape):
    return torch.full(shape, float(CANARY), dtype=torch.float32, device="cuda")


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def report(name, err, bound):
    """Largest error over bound (elements whose bound is 0 must have no error); printed, returned for the assertion."""
    err, bound = np.asarray(err, F64), np.asarray(bound, F64)
    assert np.all(err[bound == 0] == 0), f"{name}: an error where the bound is zero"
    ratio = float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0
    print(f"{name}: max err / bound = {ratio:.3f} (max abs err {float(err.max()) if err.size else 0.0:.3e})")
    return ratio


# ---- fbank ---------------------------------------------------------------------------------------------------------------------------
def pcm_of(case, s16):
    """The packed samples as the entry takes them: int16, or the float32 s / 32768.f they stand for."""
    return dev(case.pcm) if s16 else dev((case.pcm.astype(F32) / F32(32768.0)).astype(F32))


def run_raw(ops, case):
    """Raw-frames form, f32 then s16: the rows past the last frame keep the canary, the two results are equal bit for bit."""
    outs = []
    for s16 in (False, True):
        out = canary((case.total + 3, R.N_MELS))
        fo = ops.fbank_frames(pcm_of(case, s16), case.sample_off, case.n_samples, out)
        assert fo == [int(v) for v in case.frame_off]
        out = host(out)
        assert np.all(bits(out[case.total:]) == bits(CANARY)), f"{case.name}: rows past the last frame were written"
        outs.append(out[:case.total])
    assert same_bits(outs[0], outs[1]), f"{case.name}: the s16 form differs from the f32 form on s / 32768.f"
    return outs[0]


def run_fused(ops, case, mean, istd):
    """Fused form, f32 then s16, into a canary-filled buffer (tests/frontend_ref.py fused_layout): equal bit for bit."""
    row_off, rows = R.fused_layout(case)
    outs = []
    for s16 in (False, True):
        feats = canary((rows, R.FEAT))
        ops.fbank_lfr_cmvn(pcm_of(case, s16), case.sample_off, case.n_samples, row_off, dev(mean), dev(istd), feats)
        outs.append(host(feats))
    assert same_bits(outs[0], outs[1]), f"{case.name}: the fused s16 form differs from the fused f32 form"
    return outs[0], row_off, rows


def test_fbank_one_tone_per_fft_bin(ops):
    """B = 255 utterances of one frame, utterance k a tone on FFT bin k: every twiddle (the sign flip past the half turn included), every
    conjugate partner and every mel tap carries the case alone somewhere; the lookup walks four 64-entry chunks of frame_off.  Bound: 8 x
    the fp32 restatement's own largest error against fp64 on this case (1.18e-4), the median against 8 x its median.
    Measured on the MI355X: max err / bound = 0.125, median err / bound = 0.157."""
    case = R.case_tones()
    assert len(case.utts) == 255 and case.total == 255
    R.check_fbank(run_raw(ops, case), case)


@pytest.mark.parametrize("amplitude", [16384, 1])
def test_fbank_one_impulse_per_window_position(ops, amplitude):
    """B = 400 utterances of one frame, utterance i an impulse at sample i: each sample's path through the loads, the DC mean, the
    pre-emphasis hand-over between lanes and rows (samples 32, 64, .., 384 take their neighbour from the previous n1) and the window is
    seen alone.  Measured on the MI355X: amplitude 16384 max err / bound = 0.125, median 0.044; amplitude 1 max 0.113, median
    0.052."""
    case = R.case_impulses(amplitude)
    assert case.total == 400
    R.check_fbank(run_raw(ops, case), case)


def test_fbank_extremes(ops):
    """Constant 32767 and constant -32768 (every bin exactly at the floor: logf(FLT_EPSILON) bit for bit), the Nyquist square wave
    +32767 / -32768, +-1 LSB noise and full-scale uniform noise, one frame each in one batch.
    Measured on the MI355X: max err / bound = 0.117, median err / bound = 0.039."""
    case = R.case_extremes()
    got = run_raw(ops, case)
    assert np.all(bits(got[:2]) == bits(R.LOG_FLOOR))
    R.check_fbank(got, case)


COUNT_CASES = {"counts": R.case_counts, "b130": R.case_counts_130, "one": R.case_single_frame, "one_among_empty": R.case_single_frame_among_empty}


@pytest.mark.parametrize("which", list(COUNT_CASES))
def test_fbank_every_small_frame_count(ops, which):
    """Utterances of F = 1 .. 25 frames (400 + 160 (F - 1) + r samples, r cycling over 0, 1, 159; odd sample offsets in the s16 run),
    zero-frame utterances (0 and 399 samples) first and last; B = 130 with zero-frame utterances at positions 63, 64, 65 of the lookup;
    total_frames = 1 alone (the B == 1 launcher) and among empty utterances; total_frames never a multiple of 16.
    Raw frames against fp64.  Then the fused form must equal, bit for bit, pfhip_op_lfr_cmvn(m = 7, n = 6) of the raw frames of the same
    launch inputs (one rounding order for (x + mean) * istd and no contraction: nothing but equality is acceptable), canary rows
    included, and that composite must equal oracle.frontend.lfr_cmvn of the GPU frames bit for bit.
    Measured on the MI355X (max / median err over bound): counts 0.129 / 0.061, b130 0.125 / 0.062, one 0.143 / 0.068,
    one_among_empty 0.160 / 0.063."""
    case = COUNT_CASES[which]()
    assert case.total % 16
    raw = run_raw(ops, case)
    R.check_fbank(raw, case)
    mean, istd = R.cmvn_vectors()
    fused, row_off, rows = run_fused(ops, case, mean, istd)
    composite = canary((rows, R.FEAT))
    d_raw, d_mean, d_istd = dev(raw), dev(mean), dev(istd)
    for b, nf in enumerate(case.nframes):
        if nf:
            ops.lfr_cmvn(d_raw[case.frame_off[b]:], nf, 7, 6, R.N_MELS, d_mean, d_istd, composite[row_off[b]:])
    assert same_bits(fused, host(composite)), f"{case.name}: fused form != lfr_cmvn(raw frames)"
    assert R.fused_mismatches(fused, raw, case, row_off, mean, istd, CANARY) == 0


def test_fbank_refusals(ops, pkg):
    """A null pointer, B < 1, total_frames != frame_off[B], both outputs or neither, a frame outside pcm, a row outside feats: refused
    before anything is launched (the outputs keep their canary)."""
    case = R.case_single_frame_among_empty()
    pcm = pcm_of(case, True)
    nf, fo, so, B = case.nframes, [int(v) for v in case.frame_off], case.sample_off, len(case.nframes)
    out, feats = canary((4, R.N_MELS)), canary((4, R.FEAT))
    mean, istd = (dev(v) for v in R.cmvn_vectors())
    good = dict(pcm=pcm, pcm_samples=pcm.numel(), sample_off=so, frame_off=fo, nframes=nf, B=B, total_frames=fo[-1], fb_out=out)
    fused = dict(good, fb_out=None, feats=feats, feats_rows=4, row_off=[0, 0, 1], cmvn_mean=mean, cmvn_istd=istd)
    bad = [dict(good, pcm=None), dict(good, sample_off=None), dict(good, frame_off=None), dict(good, nframes=None), dict(good, B=0),
           dict(good, B=-1), dict(good, total_frames=fo[-1] + 1), dict(good, total_frames=0), dict(good, fb_out=None),
           dict(good, feats=feats, feats_rows=4, row_off=[0, 0, 1], cmvn_mean=mean, cmvn_istd=istd),
           dict(good, pcm_samples=so[1] + 399), dict(good, frame_off=[0, 1, 1, 1]), dict(good, sample_off=[0, -1, 0]),
           dict(fused, row_off=None), dict(fused, cmvn_mean=None), dict(fused, cmvn_istd=None), dict(fused, feats_rows=0),
           dict(fused, row_off=[0, 4, 0])]
    for kw in bad:
        with pytest.raises(pkg.PfhipError):
            ops.fbank_entry(**kw)
    assert np.all(bits(host(out)) == bits(CANARY)) and np.all(bits(host(feats)) == bits(CANARY))
    ops.fbank_entry(**good)
    ops.fbank_entry(**fused)
    assert np.all(bits(host(out)[1:]) == bits(CANARY)) and np.all(bits(host(feats)[1:]) == bits(CANARY))
    assert same_bits(host(feats)[:1], FE.lfr_cmvn(host(out)[:1], *R.cmvn_vectors()))


# ---- the LFR/CMVN family: exact ----------------------------------------------------------------------------------------------------------
LFR_SHAPES = [(7, 6, 80), (5, 1, 80), (4, 3, 5)]


def lfr_vectors(rng, D):
    return rng.uniform(-10, 10, D).astype(F32), rng.uniform(0.05, 2.0, D).astype(F32)


def padded(rows, ldo):
    """rows [T, D] in a [T, ldo] matrix whose pad columns are zero."""
    out = np.zeros((rows.shape[0], ldo), F32)
    out[:, :rows.shape[1]] = rows
    return out


@pytest.mark.parametrize("m,n,n_mels", LFR_SHAPES)
def test_lfr_cmvn_exact(ops, m, n, n_mels):
    """F = 1 .. 15 (F < m: every slot of the only row clamps), ldo = m n_mels and larger (pad columns zero): bit for bit a numpy gather,
    float32 add, float32 multiply; rows past ceil(F / n) keep the canary."""
    rng = np.random.default_rng(100 * m + n)
    D = m * n_mels
    mean, istd = lfr_vectors(rng, D)
    for F in range(1, 16):
        fb = rng.standard_normal((F, n_mels)).astype(F32)
        want = R.lfr_cmvn_exact(fb, mean, istd, m, n)
        for ldo in (D, D + 12):
            out = canary((want.shape[0] + 2, ldo))
            ops.lfr_cmvn(dev(fb), F, m, n, n_mels, dev(mean), dev(istd), out)
            got = host(out)
            assert same_bits(got[:want.shape[0]], padded(want, ldo)), (F, ldo)
            assert np.all(bits(got[want.shape[0]:]) == bits(CANARY)), (F, ldo)


@pytest.mark.parametrize("m,n,n_mels", LFR_SHAPES)
def test_lfr_cmvn_packed_exact(ops, m, n, n_mels):
    """Files of 0, 1 and many frames in one launch (the launch's max_T is above most files' T), each padded at its own edges; the row
    reserved for a zero-frame file and the spare rows between files keep the canary; pad columns zero."""
    rng = np.random.default_rng(200 * m + n)
    D, ldo = m * n_mels, m * n_mels + 4
    mean, istd = lfr_vectors(rng, D)
    nframes = [0, 1, 13, 0, 7, 1, 31, 0]
    frame_off = [int(v) for v in np.concatenate([[0], np.cumsum(nframes)[:-1]])]
    fb = rng.standard_normal((sum(nframes), n_mels)).astype(F32)
    row_off, r = [], 0
    for nf in nframes:
        row_off.append(r)
        r += (nf + n - 1) // n + 1
    want = np.full((r + 2, ldo), CANARY, F32)
    for b, nf in enumerate(nframes):
        rows = R.lfr_cmvn_exact(fb[frame_off[b]:frame_off[b] + nf], mean, istd, m, n)
        want[row_off[b]:row_off[b] + rows.shape[0]] = padded(rows, ldo)
    out = canary(want.shape)
    ops.lfr_cmvn_packed(dev(fb), frame_off, nframes, row_off, m, n, n_mels, dev(mean), dev(istd), out)
    assert same_bits(host(out), want)


@pytest.mark.parametrize("m,n,n_mels", LFR_SHAPES)
def test_lfr_cmvn_online_batch_exact(ops, m, n, n_mels):
    """Operations with Tin < m (the tail replicated from the first row on), with n_out = 0, with more rows than frames, and with
    row_off scattered and out of order; no left padding.  Bit for bit; untouched rows keep the canary."""
    rng = np.random.default_rng(300 * m + n)
    D, ldo = m * n_mels, m * n_mels + 8
    mean, istd = lfr_vectors(rng, D)
    Tin = [1, m - 1 if m > 1 else 1, 3, 20, 9, m]
    n_out = [1, 2, 0, 4, 3, 1]
    row_off = [9, 0, 5, 11, 3, 7]
    fb_off, pos = [], 1
    for t in Tin:
        fb_off.append(pos)
        pos += t + 1
    fb = rng.standard_normal((pos, n_mels)).astype(F32)
    want = np.full((17, ldo), CANARY, F32)
    for k in range(len(Tin)):
        rows = R.lfr_cmvn_exact(fb[fb_off[k]:fb_off[k] + Tin[k]], mean, istd, m, n, left_pad=0, n_out=n_out[k])
        want[row_off[k]:row_off[k] + n_out[k]] = padded(rows, ldo)
    out = canary(want.shape)
    ops.lfr_cmvn_online_batch(dev(fb), fb_off, Tin, n_out, row_off, m, n, n_mels, dev(mean), dev(istd), out)
    assert same_bits(host(out), want)


def test_lfr_family_refusals(ops, pkg):
    """ldo below m n_mels, m / n / n_mels < 1, an operation with rows but no frame, rows outside the output: refused."""
    rng = np.random.default_rng(5)
    fb, mean, istd = dev(rng.standard_normal((8, 5)).astype(F32)), dev(np.zeros(20, F32)), dev(np.ones(20, F32))
    out = canary((8, 20))
    for args in [(fb, 8, 5, 3, 5, mean, istd, out), (fb, 8, 0, 3, 5, mean, istd, out), (fb, 8, 4, 0, 5, mean, istd, out),
                 (fb, -1, 4, 3, 5, mean, istd, out), (None, 8, 4, 3, 5, mean, istd, out)]:
        with pytest.raises(pkg.PfhipError):
            ops.lfr_cmvn(*args)
    with pytest.raises(pkg.PfhipError):
        ops.lfr_cmvn_online_batch(fb, [0], [0], [1], [0], 4, 3, 5, mean, istd, out)
    with pytest.raises(pkg.PfhipError):
        ops.lfr_cmvn_online_batch(fb, [0], [8], [9], [0], 4, 3, 5, mean, istd, out)
    with pytest.raises(pkg.PfhipError):
        ops.lfr_cmvn_packed(fb, [0], [9], [0], 4, 3, 5, mean, istd, out)
    with pytest.raises(pkg.PfhipError):
        ops.lfr_cmvn_packed(fb, [0], [8], [6], 4, 3, 5, mean, istd, out)
    assert np.all(bits(host(out)) == bits(CANARY))


def test_rows_copy_batch_exact(ops, pkg):
    """Operations of different sizes in one launch: a plain copy with ncols < ldd (pad columns zero), no source (zeros), lds == 0 (row 0
    repeated), nrows = 0 (nothing written), one row; everything between the operations keeps the canary."""
    rng = np.random.default_rng(77)
    src = rng.standard_normal(4000).astype(F32)
    #        dst_off src_off ldd lds nrows ncols
    spec = [(10, 0, 24, 30, 5, 20),
            (200, -1, 16, 0, 3, 16),
            (300, 500, 40, 0, 6, 33),
            (700, 900, 8, 8, 0, 8),
            (800, 1000, 80, 80, 1, 80),
            (1000, 2000, 560, 560, 2, 560)]
    want = np.full(2200, CANARY, F32)
    for d_off, s_off, ldd, lds, nrows, ncols in spec:
        for r in range(nrows):
            row = np.zeros(ldd, F32)
            if s_off >= 0:
                row[:ncols] = src[s_off + r * lds:s_off + r * lds + ncols]
            want[d_off + r * ldd:d_off + (r + 1) * ldd] = row
    dst = canary((2200,))
    cols = list(zip(*spec))
    ops.rows_copy_batch(dst, cols[0], dev(src), cols[1], cols[2], cols[3], cols[4], cols[5])
    assert same_bits(host(dst), want)
    before = host(dst).copy()
    for bad in [([0], [0], [8], [8], [1], [9]), ([2195], [0], [8], [8], [1], [8]), ([0], [3995], [8], [8], [1], [8]), ([0], [0], [8], [4], [2], [8])]:
        with pytest.raises(pkg.PfhipError):
            ops.rows_copy_batch(dst, bad[0], dev(src), bad[1], bad[2], bad[3], bad[4], bad[5])
    with pytest.raises(pkg.PfhipError):
        ops.rows_copy_batch(dst, [0], None, [0], [8], [8], [1], [8])          # a source offset without a source
    assert same_bits(host(dst), before)


# ---- the positional-encoding kernels ---------------------------------------------------------------------------------------------------
# The one inexact step is the device sinf / cosf.  The ROCm headers and documents beside the compiler state no ulp bound for them, so it
# is measured: test_device_sincos_ulp runs the embed kernel on zero features (its output is then the sine / cosine itself) over the
# positions and widths of these tests; the worst error found was 1.165 ulp of the result, and the bound is twice that.
SINCOS_ULP = 2.33
POSITIONS = [0, 1, 499, 5000, 1_000_000]


def pe_bound(exact, pe):
    """SINCOS_ULP ulp of the sine / cosine, plus one ulp of the result for the final add (fl32(x * scale) is exact in the reference)."""
    return SINCOS_ULP * R.ulp32(pe) + R.ulp32(exact)


@pytest.mark.parametrize("D", [560, 512, 256])
def test_device_sincos_ulp(ops, D):
    """embed on zero features: x0 = sinf / cosf(fl32(inv_ts * pos)) exactly, for positions 0, 1, 499, 5000 and 1 000 000 (+ 1) and every
    timescale of the width.  Error in ulp of the fp64 sine / cosine.  Measured on the MI355X: worst 1.165 ulp (bound
    SINCOS_ULP = twice that)."""
    inv = R.inv_timescales(D)
    pos = np.array(POSITIONS, np.int32)
    x0 = canary((len(pos), D))
    ops.embed(dev(np.zeros((len(pos), D), F32)), D, x0, dev(pos), len(pos), dev(inv), 3.0)
    pe = R.pe64(inv, pos + 1, D)
    err = np.abs(host(x0).astype(F64) - pe) / R.ulp32(pe)
    print(f"D = {D}: device sinf / cosf worst error {err.max():.3f} ulp")
    assert err.max() <= SINCOS_ULP


@pytest.mark.parametrize("D,ldx", [(560, 576), (512, 512), (256, 256)])
def test_embed(ops, D, ldx):
    """x0 = feats * sqrt(D) + PE(row_pos + 1) with non-monotonic row_pos (0, 1, 499, 5000, 1 000 000 among them), pad columns D .. ldx
    zero, rows past M untouched.  Measured on the MI355X: max err / bound = 0.500 (D = 512; 0.499 at 560, 0.496 at 256)."""
    rng = np.random.default_rng(D)
    pos = np.array([5000, 0, 1_000_000, 1, 499, 37, 36, 0, 123456, 2], np.int32)
    M = len(pos)
    inv, scale = R.inv_timescales(D), F32(np.sqrt(F32(D)))
    feats = rng.standard_normal((M, D)).astype(F32)
    x0 = canary((M + 2, ldx))
    ops.embed(dev(feats), D, x0, dev(pos), M, dev(inv), scale)
    got = host(x0)
    pe = R.pe64(inv, pos + 1, D)
    _, exact = R.embed_ref(feats, scale, pe)
    assert np.all(got[:M, D:] == 0) and np.all(bits(got[M:]) == bits(CANARY))
    assert report(f"embed D = {D}", np.abs(got[:M, :D].astype(F64) - exact), pe_bound(exact, pe)) <= 1.0


@pytest.mark.parametrize("D,Dout,ldo", [(256, 256, 256), (512, 512, 520), (516, 544, 560)])
@pytest.mark.parametrize("with_pos", [False, True])
def test_embed_gather(ops, D, Dout, ldo, with_pos):
    """out = table[id] * sqrt(D) + PE: ids at -1, 0, vocab - 1 and vocab among ordinary ones — the kernel CLAMPS an id to [0, vocab - 1]
    (asserted: -1 reads row 0, vocab reads row vocab - 1); pos_of_row null (the row index) and given (non-monotonic, up to 1 000 000);
    columns D .. Dout zero, columns Dout .. ldo and rows past N untouched.  Measured on the MI355X: max err / bound = 0.500."""
    rng = np.random.default_rng(D + with_pos)
    vocab = 23
    table = rng.standard_normal((vocab, D)).astype(F32)
    ids = np.array([-1, 0, vocab - 1, vocab, 7, 7, 3, -2_000_000_000, 2_000_000_000, 11], np.int32)
    N = len(ids)
    pos = np.array([499, 0, 5000, 1, 1_000_000, 0, 36, 35, 2, 77], np.int32) if with_pos else np.arange(N, dtype=np.int32)
    inv, scale = R.inv_timescales(D), F32(np.sqrt(F32(D)))
    out = canary((N + 2, ldo))
    ops.embed_gather(dev(ids), dev(table), D, Dout, out, N, dev(inv), scale, dev(pos) if with_pos else None)
    got = host(out)
    pe = R.pe64(inv, pos + 1, D)
    _, exact = R.embed_ref(table[np.clip(ids, 0, vocab - 1)], scale, pe)
    assert np.all(got[:N, D:Dout] == 0) and np.all(bits(got[:N, Dout:]) == bits(CANARY)) and np.all(bits(got[N:]) == bits(CANARY))
    assert report(f"embed_gather D = {D}", np.abs(got[:N, :D].astype(F64) - exact), pe_bound(exact, pe)) <= 1.0


def test_stream_lfr_batch(ops):
    """Connections of T = 1 .. 13 frames (the tail replicated with the last frame) and pos0 of 0, 499, 5000 and 1 000 000 in one launch,
    rows scattered; LFR + CMVN exact in fp32, then fl32(x * scale) + PE.  Columns 560 .. ldo = 576 and unused rows keep the canary.
    Measured on the MI355X: max err / bound = 0.500."""
    rng = np.random.default_rng(13)
    mean, istd = lfr_vectors(rng, 560)
    inv, scale = R.inv_timescales(560), F32(np.sqrt(F32(512)))
    T = list(range(1, 14))
    n_rows = [max(1, (t + 5) // 6) + (1 if t % 4 == 0 else 0) for t in T]        # some ask for a row that is all tail
    pos0 = [POSITIONS[k % 4 + 1] if k % 5 else 0 for k in range(len(T))]
    fb_off, p = [], 0
    for t in T:
        fb_off.append(p)
        p += t
    fb = rng.standard_normal((p, 80)).astype(F32)
    order = rng.permutation(len(T))
    row_off, r = [0] * len(T), 1
    for k in order:
        row_off[k] = r
        r += n_rows[k] + 1
    out = canary((r + 1, 576))
    ops.stream_lfr_batch(dev(fb), fb_off, T, n_rows, pos0, row_off, dev(mean), dev(istd), scale, dev(inv), out)
    got = host(out)
    written = np.zeros(got.shape, bool)
    worst = 0.0
    for k, t in enumerate(T):
        x = R.lfr_cmvn_exact(fb[fb_off[k]:fb_off[k] + t], mean, istd, 7, 6, left_pad=0, n_out=n_rows[k])
        pe = R.pe64(inv, pos0[k] + 1 + np.arange(n_rows[k]), 560)
        _, exact = R.embed_ref(x, scale, pe)
        rows = slice(row_off[k], row_off[k] + n_rows[k])
        written[rows, :560] = True
        worst = max(worst, report(f"stream_lfr T = {t} pos0 = {pos0[k]}", np.abs(got[rows, :560].astype(F64) - exact), pe_bound(exact, pe)))
    assert np.all(bits(got[~written]) == bits(CANARY))
    assert worst <= 1.0


def test_pe_refusals(ops, pkg):
    x0 = canary((2, 16))
    z, pos, inv = dev(np.zeros((2, 16), F32)), dev(np.zeros(2, np.int32)), dev(np.ones(8, F32))
    for D, buf in [(15, x0), (0, x0), (16, canary((2, 12)))]:
        with pytest.raises(pkg.PfhipError):
            ops.embed(z, D, buf, pos, 2, inv, 1.0)
    with pytest.raises(pkg.PfhipError):
        ops.embed_gather(pos, z, 16, 20, x0, 2, inv, 1.0)                       # Dout above ldo
    with pytest.raises(pkg.PfhipError):
        ops.stream_lfr_batch(z, [0], [0], [1], [0], [0], inv, inv, 1.0, inv, canary((2, 576)))      # rows but no frame
    assert np.all(bits(host(x0)) == bits(CANARY))
