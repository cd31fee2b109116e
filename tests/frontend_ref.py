"""TEST INFRASTRUCTURE: fp64 / exact references of the front-end kernels (csrc/fbank.hip, vad.hip, stream.hip, punc.hip), the fbank
cases of tests/test_gpu_frontend_ops.py and the comparison those cases are judged by.

The references use the chain's own fp32-VALUED constants widened to fp64 (oracle.frontend.hamming_window(), the mel_banks() weights,
0.97f), so that a difference from them is arithmetic and nothing else.  The cases and the comparison live here, not in the GPU test,
because tests/test_frontend_ref.py runs the same comparison on the CPU over a numpy restatement of the kernel with seeded defects: the
check that the GPU tests would notice a subtly wrong kernel.
"""
import functools

import numpy as np

from oracle import frontend as FE

F32, F64 = np.float32, np.float64
FLT_EPS = F64(np.finfo(F32).eps)
LOG_FLOOR = F32(FE._logf(np.finfo(F32).eps))          # logf(FLT_EPSILON), what the kernel writes for an energy at the floor
N_MELS, FLEN, FSHIFT, NFFT = 80, 400, 160, 512


@functools.lru_cache(maxsize=None)
def mel_matrix():
    """[80, 257] fp64: the fp32 mel weights of the chain, widened."""
    off, size, w = FE.mel_banks(N_MELS)
    m = np.zeros((N_MELS, NFFT // 2 + 1), F64)
    for b in range(N_MELS):
        m[b, off[b]:off[b] + size[b]] = w[b].astype(F64)
    return m


def frames_of(x, n_frames):
    """[n_frames, 400] windows of one utterance's samples."""
    idx = np.arange(n_frames)[:, None] * FSHIFT + np.arange(FLEN)[None, :]
    return np.asarray(x)[idx]


def fbank64(frames):
    """Plain fp64 fbank of a [n, 400] matrix of integer-valued samples (the x 32768 scale): DC removal, pre-emphasis, window, 512-point
    rfft, power, mel sums, log(max(e, FLT_EPSILON)).  Returns (log-mel [n, 80], mel energies [n, 80]), both fp64."""
    x = np.asarray(frames, F64)
    assert x.ndim == 2 and x.shape[1] == FLEN
    d = x - x.mean(axis=1, keepdims=True)
    pre = F64(FE.PREEMPH)
    y = np.empty_like(d)
    y[:, 1:] = d[:, 1:] - pre * d[:, :-1]
    y[:, 0] = d[:, 0] - pre * d[:, 0]
    y *= FE.hamming_window().astype(F64)[None, :]
    spec = np.fft.rfft(y, NFFT, axis=1)
    e = (spec.real ** 2 + spec.imag ** 2) @ mel_matrix().T
    return np.log(np.maximum(e, FLT_EPS)), e


def restatement32(samples_i16):
    """oracle.frontend.fbank (the fp32 restatement the whole-model tests compare with) of one utterance of 16-bit samples."""
    return FE.fbank((np.asarray(samples_i16, F32) / F32(32768.0)).astype(F32))


def lfr_rows(F, m, n, left_pad=None, n_out=None):
    """Frame index [T, m] that row i, slot j of LfrCmvn reads: i n + j - left_pad clamped to [0, F - 1].  left_pad (m - 1) / 2 is the
    offline routine, 0 with n_out rows the online one."""
    lp = (m - 1) // 2 if left_pad is None else left_pad
    T = (F + n - 1) // n if n_out is None else n_out
    f = np.arange(T)[:, None] * n + np.arange(m)[None, :] - lp
    return np.clip(f, 0, max(F - 1, 0))


def lfr_cmvn_exact(fb, mean, istd, m, n, left_pad=None, n_out=None):
    """LfrCmvn exactly: a gather, then a float32 add, then a float32 multiply.  fb [F, n_mels] float32 -> [T, m n_mels] float32."""
    fb = np.asarray(fb, F32)
    idx = lfr_rows(fb.shape[0], m, n, left_pad, n_out)
    if idx.shape[0] == 0:
        return np.zeros((0, m * fb.shape[1]), F32)
    g = fb[idx].reshape(idx.shape[0], -1)
    return ((g + np.asarray(mean, F32)[None, :]).astype(F32) * np.asarray(istd, F32)[None, :]).astype(F32)


def inv_timescales(D):
    """The fp32 inverse timescales the loaders upload for width D (oracle.frontend.pos_emb's)."""
    half = D // 2
    scale = F32(-np.log(10000.0) / (half - 1)) if D != 560 else FE.PE_SCALE
    return np.exp((np.arange(half, dtype=F32) * scale).astype(F32).astype(F64)).astype(F32)


def pe64(inv_ts, pos, D):
    """[len(pos), D] fp64: sin | cos of coe32 = fl32(inv_ts32 * (float)pos), the sine and cosine themselves in fp64."""
    coe = (np.asarray(inv_ts, F32)[None, :] * np.asarray(pos, F32)[:, None]).astype(F32).astype(F64)
    return np.concatenate([np.sin(coe), np.cos(coe)], axis=1)


def embed_ref(x, scale, pe):
    """(reference fl32(fl32(x * scale) + pe) with pe in fp64, the sum before its rounding in fp64)."""
    xs = (np.asarray(x, F32) * F32(scale)).astype(F32).astype(F64)
    return (xs + pe).astype(F32), xs + pe


def ulp32(v):
    """The spacing of float32 at |v| (fp64 array)."""
    return np.spacing(np.abs(np.asarray(v, F64)).astype(F32)).astype(F64)


def logsumexp64(x):
    """Row log-sum-exp in fp64; a row that is all -inf gives -inf."""
    x = np.asarray(x, F64)
    m = x.max(axis=1)
    safe = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return safe + np.log(np.exp(x - safe[:, None]).sum(axis=1))


# ---- fbank cases ---------------------------------------------------------------------------------------------------------------------
class FbankCase:
    """Utterances of 16-bit samples packed back to back (with `gap` unused samples in front of each, so that s16 offsets are odd where
    the gaps are), the fp64 reference of every frame and the fp32 restatement's own error against it."""

    def __init__(self, name, utts, gaps=None):
        self.name = name
        self.utts = [np.asarray(u, np.int16) for u in utts]
        gaps = [0] * len(utts) if gaps is None else gaps
        self.n_samples = [len(u) for u in self.utts]
        self.sample_off, parts, pos = [], [], 0
        for u, g in zip(self.utts, gaps):
            parts.append(np.full(g, 12345, np.int16))            # samples no frame may read
            pos += g
            self.sample_off.append(pos)
            parts.append(u)
            pos += len(u)
        self.pcm = np.concatenate(parts) if parts else np.zeros(0, np.int16)
        self.nframes = [FE.num_frames(n) for n in self.n_samples]
        self.frame_off = [0] + list(np.cumsum(self.nframes))
        self.total = int(self.frame_off[-1])
        refs, ens, e32 = [], [], []
        for u, nf in zip(self.utts, self.nframes):
            if nf == 0:
                continue
            r, e = fbank64(frames_of(u.astype(F64), nf))
            refs.append(r)
            ens.append(e)
            e32.append(np.abs(restatement32(u).astype(F64) - r))
        self.ref, self.energy, self.e32 = np.concatenate(refs), np.concatenate(ens), np.concatenate(e32)
        assert self.ref.shape == (self.total, N_MELS)

    @property
    def floor(self):
        return self.energy <= FLT_EPS


FACTOR = 8.0      # the bound over the restatement's own error, and the floor in ulps (tests/test_gpu_blstm_op.py's reasoning: a
                  # differently ordered fp32 sum, here the 16-lane tree of the DC mean, against the restatement's sequential one)


def fbank_ratios(got, case):
    """(largest error over bound, median error over its bound, number of floor elements that are not logf(FLT_EPSILON) exactly).
    Bound per element: FACTOR x the restatement's largest error on this case, at least FACTOR ulp of the reference value.  Median:
    FACTOR x the restatement's median error, at least FACTOR ulp of the median |reference|.  Floor elements (fp64 energy at or below
    FLT_EPSILON) are judged by exact equality alone."""
    got = np.asarray(got)
    assert got.dtype == F32 and got.shape == case.ref.shape, (got.dtype, got.shape, case.ref.shape)
    fl = case.floor
    bad_floor = int(np.count_nonzero(got[fl] != LOG_FLOOR))
    if np.all(fl):
        return 0.0, 0.0, bad_floor
    err = np.abs(got.astype(F64) - case.ref)[~fl]
    if not np.all(np.isfinite(err)):
        return np.inf, np.inf, bad_floor
    ref, e32 = case.ref[~fl], case.e32[~fl]
    bound = np.maximum(FACTOR * e32.max(), FACTOR * ulp32(ref))
    med_bound = max(FACTOR * float(np.median(e32)), FACTOR * float(ulp32(np.median(np.abs(ref)))))
    return float((err / bound).max()), float(np.median(err)) / med_bound, bad_floor


def check_fbank(got, case):
    """Prints error over bound, asserts all three; returns the two ratios."""
    r_max, r_med, bad_floor = fbank_ratios(got, case)
    print(f"{case.name}: max err / bound = {r_max:.3f}, median err / bound = {r_med:.3f}, floor elements off: {bad_floor} of "
          f"{int(case.floor.sum())} (restatement vs fp64: max {case.e32.max():.2e}, median {np.median(case.e32):.2e})")
    assert bad_floor == 0, f"{case.name}: {bad_floor} elements at the floor are not logf(FLT_EPSILON)"
    assert r_max <= 1.0, f"{case.name}: max err / bound = {r_max:.3f}"
    assert r_med <= 1.0, f"{case.name}: median err / bound = {r_med:.3f}"
    return r_max, r_med


@functools.lru_cache(maxsize=None)
def case_tones():
    """One tone per FFT bin: B = 255 utterances of exactly 400 samples, utterance k = round(8000 cos(2 pi k n / 512 + 0.3))."""
    n = np.arange(FLEN)
    return FbankCase("tones", [np.round(8000.0 * np.cos(2 * np.pi * k * n / 512.0 + 0.3)) for k in range(1, 256)])


@functools.lru_cache(maxsize=None)
def case_impulses(amplitude):
    """One impulse per window position: B = 400 utterances, utterance i = amplitude at sample i, 0 elsewhere."""
    return FbankCase(f"impulses of {amplitude}", list(np.eye(FLEN) * amplitude))


@functools.lru_cache(maxsize=None)
def case_extremes():
    rng = np.random.default_rng(20261020)
    nyq = np.where(np.arange(FLEN) % 2 == 0, 32767, -32768)
    return FbankCase("extremes", [np.full(FLEN, 32767), np.full(FLEN, -32768), nyq, rng.integers(-1, 2, FLEN),
                                  rng.integers(-32768, 32768, FLEN)])


def _speechlike(rng, n):
    t = np.arange(n) / 16000.0
    x = 8000.0 * (0.6 * np.sin(2 * np.pi * rng.uniform(90, 400) * t) + 0.4 * rng.standard_normal(n))
    return np.clip(np.round(x), -32768, 32767)


def _counts_case(name, seed, frame_counts):
    """frame_counts: F per utterance; F = 0 alternates between 0 and 399 samples.  Sample counts 400 + 160 (F - 1) + r with r cycling
    over 0, 1, 159; gaps of 0 / 1 samples in front of the utterances make odd sample offsets."""
    rng = np.random.default_rng(seed)
    utts, gaps, empties = [], [], 0
    for i, F in enumerate(frame_counts):
        if F == 0:
            n = (0, 399)[empties % 2]
            empties += 1
        else:
            n = FLEN + FSHIFT * (F - 1) + (0, 1, 159)[i % 3]
        utts.append(_speechlike(rng, n))
        gaps.append(i % 2)
    return FbankCase(name, utts, gaps)


@functools.lru_cache(maxsize=None)
def case_counts():
    """Every small frame count, F = 1 .. 25, a zero-frame utterance first and last: 27 utterances, 325 frames."""
    c = _counts_case("frame counts 1..25", 11, [0] + list(range(1, 26)) + [0])
    assert c.total % 16 and any(o % 2 for o in c.sample_off)
    return c


@functools.lru_cache(maxsize=None)
def case_counts_130():
    """B = 130 (three chunks of the frame_off lookup): zero-frame utterances (0 and 399 samples) at positions 63, 64 and 65."""
    counts = [1 + (5 * i) % 9 for i in range(130)]
    for i in (63, 64, 65):
        counts[i] = 0
    c = _counts_case("B = 130 with empty utterances at 63..65", 12, counts)
    assert c.total % 16
    return c


@functools.lru_cache(maxsize=None)
def case_single_frame():
    """total_frames = 1: one utterance of one frame (the B == 1 launcher)."""
    return _counts_case("one frame", 13, [1])


@functools.lru_cache(maxsize=None)
def case_single_frame_among_empty():
    """total_frames = 1 in a batch: empty, one frame, empty."""
    return _counts_case("one frame among empty utterances", 14, [0, 1, 0])


# ---- the fused LFR scatter: layout and comparison ------------------------------------------------------------------------------------
FEAT = 7 * N_MELS


def cmvn_vectors():
    """Non-trivial CMVN vectors: mean in [-10, 10], istd in [0.05, 2]."""
    rng = np.random.default_rng(560)
    return rng.uniform(-10, 10, FEAT).astype(F32), rng.uniform(0.05, 2.0, FEAT).astype(F32)


def fused_layout(case):
    """(row_off per utterance, rows of the buffer): every utterance's ceil(F / 6) rows, one spare row after each, three at the end."""
    row_off, r = [], 0
    for nf in case.nframes:
        row_off.append(r)
        r += (nf + 5) // 6 + 1
    return row_off, r + 3


def fused_mismatches(feats, raw, case, row_off, mean, istd, canary):
    """Elements of the fused output [rows, 560] that differ, bit for bit, from oracle.frontend.lfr_cmvn of the utterance's raw frames
    (`raw` [total, 80], the same kernel's raw-frames output) or, outside every utterance's rows, from the canary."""
    want = np.full(feats.shape, canary, F32)
    for b, nf in enumerate(case.nframes):
        if nf:
            rows = FE.lfr_cmvn(raw[case.frame_off[b]:case.frame_off[b + 1]], mean, istd)
            assert np.array_equal(rows, lfr_cmvn_exact(raw[case.frame_off[b]:case.frame_off[b + 1]], mean, istd, 7, 6))
            want[row_off[b]:row_off[b] + rows.shape[0]] = rows
    return int(np.count_nonzero(feats.view(np.uint32) != want.view(np.uint32)))
