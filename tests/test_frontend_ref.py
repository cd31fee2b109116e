"""CPU: the fp64 front-end references of tests/frontend_ref.py against the fp32 restatement (oracle/frontend.py), and the sensitivity
of the GPU tests' comparison: a numpy restatement of csrc/fbank.hip's arithmetic, lane for lane where it matters (the per-lane sums and
the 16-lane tree of the DC mean, the pre-emphasis neighbour hand-over, the 16 x 16 transform with its twiddle sign flip, the conjugate
partner of the real-input split, the mel taps, the frame-to-utterance lookup, the LFR scatter), with switchable seeded defects, run
through the comparison code the GPU tests use.  Nothing here needs a GPU.
"""
import numpy as np
import pytest

import frontend_ref as R
from oracle import frontend as FE

F32, F64 = np.float32, np.float64
CANARY = F32(-1234.5)

# The restatement's own largest error against fp64 per input family, measured on the CPU (log-mel, one 400-sample frame each)
E32_TABLE = {"tones": 1.2e-4, "impulses": 9.2e-6, "noise": 7.7e-5, "lsb": 2.3e-5, "nyquist": 1.4e-5, "constant": 4.3e-7}


def test_restatement_error_per_family():
    """The fp32 restatement agrees with the fp64 reference within twice the figure measured for each input family (E32_TABLE): an
    ill-conditioned input, or a reference that drifted from the chain, fails here and not as a mystery on the GPU.  Broadband
    multi-frame utterances (the frame-count cases) are held to the full-scale-noise figure."""
    fams = [("tones", R.case_tones().e32), ("impulses", R.case_impulses(16384).e32)]
    ex = R.case_extremes().e32
    fams += [("constant", ex[0:2]), ("nyquist", ex[2:3]), ("lsb", ex[3:4]), ("noise", ex[4:5]),
             ("noise", R.case_counts().e32), ("noise", R.case_counts_130().e32)]
    for name, e in fams:
        print(f"{name}: restatement vs fp64 max {e.max():.2e}, median {np.median(e):.2e} (table {E32_TABLE[name]:.1e})")
    for name, e in fams:
        assert e.max() <= 2 * E32_TABLE[name], (name, float(e.max()))


def test_floor_elements():
    """Constant inputs leave all 80 energies exactly at the floor in fp64 (and nothing else in the extremes case does)."""
    c = R.case_extremes()
    assert np.all(c.floor[0:2]) and not np.any(c.floor[2:])
    assert np.all(c.energy[0:2] == 0.0)


def test_lfr_cmvn_exact_is_the_oracle():
    rng = np.random.default_rng(3)
    mean, istd = R.cmvn_vectors()
    for F in range(1, 30):
        fb = rng.standard_normal((F, 80)).astype(F32)
        assert np.array_equal(R.lfr_cmvn_exact(fb, mean, istd, 7, 6), FE.lfr_cmvn(fb, mean, istd))
    fb = rng.standard_normal((9, 5)).astype(F32)
    got = R.lfr_cmvn_exact(fb, np.zeros(20, F32), np.ones(20, F32), 4, 3)
    assert got.shape == (3, 20)
    assert np.array_equal(got[0, :5], fb[0]) and np.array_equal(got[0, 5:10], fb[0]) and np.array_equal(got[0, 10:15], fb[1])
    assert np.array_equal(got[2, 15:], fb[8])
    on = R.lfr_cmvn_exact(fb, np.zeros(20, F32), np.ones(20, F32), 4, 3, left_pad=0, n_out=3)
    assert np.array_equal(on[0, :5], fb[0]) and np.array_equal(on[0, 5:10], fb[1]) and np.array_equal(on[2, 15:], fb[8])


def test_pe_and_logsumexp_references():
    inv = R.inv_timescales(560)
    pe = R.pe64(inv, [1, 2, 500], 560)
    assert np.abs(pe - FE.pos_emb(500, 560)[[0, 1, 499]]).max() < 2e-7          # the oracle's table is the fp32 rounding of this
    assert pe.shape == (3, 560) and pe[0, 0] == np.sin(1.0) and pe[0, 280] == np.cos(1.0)
    x = np.array([[0.0, -np.inf, np.log(3.0)], [-np.inf] * 3, [80.0, -80.0, 80.0]])
    lse = R.logsumexp64(x)
    assert abs(lse[0] - np.log(4.0)) < 1e-15 and lse[1] == -np.inf and abs(lse[2] - (80.0 + np.log(2.0))) < 1e-13


# ---- the kernel's arithmetic in numpy, with seeded defects -------------------------------------------------------------------------------
# 1 the last tap of one mel triangle dropped                  5 the conjugate partner read at k, not at 256 - k
# 2 pre-emphasis neighbour of sample 32 n1 from the same n1   6 the DC mean divided by 512, not by 400
# 3 d[0] - 0.97 d[0] replaced by d[0]                         7 LFR scatter right edge `>= F + 2` for `> F + 2` (an EQUIVALENT mutant)
# 4 twiddle sign flip for j >= 128 omitted                    8 frame-to-utterance lookup off by one after an empty utterance
# 9 (added, the nearest mutant of 7 that changes anything) the right edge written `> F + 3`
DROPPED_TAP_BIN = 40


def sim_frames_of_windows(x, defect=0):
    """x [n, 400] float32 integer-valued windows -> log-mel [n, 80] float32, csrc/fbank.hip's arithmetic."""
    n = x.shape[0]
    xp = np.zeros((n, 416), F32)
    xp[:, :400] = x
    lanes = xp.reshape(n, 13, 16, 2)                                   # [n1][l][even / odd]: sample 32 n1 + 2 l (+ 1)
    s = np.zeros((n, 16), F32)
    for n1 in range(13):
        s = s + lanes[:, n1, :, 0]
        s = s + lanes[:, n1, :, 1]
    for off in (8, 4, 2, 1):
        s = s + s[:, np.arange(16) ^ off]
    assert np.all(s == s[:, :1])
    mean = s[:, 0] / F32(512.0 if defect == 6 else 400.0)
    d = (x - mean[:, None]).astype(F32)
    prev = np.empty_like(d)
    prev[:, 1:] = d[:, :-1]
    prev[:, 0] = d[:, 0]
    if defect == 2:
        for n1 in range(1, 13):                                        # lane 15's odd sample of the SAME n1 (zero padding - mean past 400)
            prev[:, 32 * n1] = d[:, 32 * n1 + 31] if 32 * n1 + 31 < 400 else (F32(0) - mean)
    y = d - (F32(0.97) * prev).astype(F32)
    if defect == 3:
        y[:, 0] = d[:, 0]
    y = (y * FE.hamming_window()[None, :]).astype(F32)
    z = np.zeros((n, 256), np.complex128)
    z[:, :200] = y[:, 0::2].astype(F64) + 1j * y[:, 1::2].astype(F64)
    u = z.reshape(n, 16, 16)                                           # [n1][n2]
    A = np.fft.fft(u, axis=1)                                          # n1 -> k1
    k1, n2 = np.arange(16)[:, None], np.arange(16)[None, :]
    j = k1 * n2
    tw = np.exp(-2j * np.pi * np.arange(256) / 512.0)
    w = tw[(2 * j) & 255]
    if defect != 4:
        w = np.where(j >= 128, -w, w)
    Z = np.fft.fft(A * w[None], axis=2)                                # n2 -> k2; Z[k1 + 16 k2]
    Z = Z.transpose(0, 2, 1).reshape(n, 256)
    k = np.arange(256)
    zn = Z[:, k] if defect == 5 else Z[:, (256 - k) & 255]
    e = 0.5 * (Z + np.conj(zn))
    o = -0.5j * (Z - np.conj(zn))
    X = e + tw[None] * o
    re, im = X.real.astype(F32), X.imag.astype(F32)
    ps = ((re * re).astype(F32) + (im * im).astype(F32)).astype(F32)
    offs, sizes, weights = FE.mel_banks(80)
    out = np.empty((n, 80), F32)
    for b in range(80):
        acc = np.zeros(n, F32)
        taps = int(sizes[b]) - (1 if defect == 1 and b == DROPPED_TAP_BIN else 0)
        for t in range(taps):
            acc = (acc + (weights[b][t] * ps[:, offs[b] + t]).astype(F32)).astype(F32)
        out[:, b] = acc
    at_floor = out <= np.finfo(F32).eps
    res = np.log(np.maximum(out, np.finfo(F32).eps)).astype(F32)
    res[at_floor] = R.LOG_FLOOR
    return res


def sim_lookup(case, defect=0):
    """(utterance, frame inside it) of every global frame: the kernel's count of frame_off entries at or below the frame."""
    fo = np.asarray(case.frame_off[:-1])
    g = np.arange(case.total)
    b = (fo[None, :] <= g[:, None]).sum(axis=1) - 1
    if defect == 8:
        nf = np.asarray(case.nframes)
        b = np.where((b >= 1) & (nf[np.maximum(b - 1, 0)] == 0), b - 1, b)
    return b, g - fo[b]


def sim_raw(case, defect=0):
    b, f = sim_lookup(case, defect)
    pcm = np.concatenate([case.pcm.astype(F32), np.zeros(R.FLEN, F32)])
    start = np.asarray(case.sample_off)[b] + f * R.FSHIFT
    return sim_frames_of_windows(pcm[start[:, None] + np.arange(R.FLEN)[None, :]], defect)


def sim_fused(case, raw, row_off, rows, mean, istd, defect=0):
    """The kernel's LFR scatter + CMVN of the frames `raw` into a canary-filled [rows, 560]."""
    feats = np.full((rows, R.FEAT), CANARY, F32)
    edge = {7: lambda v, F: v >= F + 2, 9: lambda v, F: v > F + 3}.get(defect, lambda v, F: v > F + 2)
    bs, fs = sim_lookup(case, defect)
    for g, (b, f) in enumerate(zip(bs, fs)):
        F = case.nframes[b]
        T = (F + 5) // 6

        def emit(t, j):
            c = slice(j * 80, (j + 1) * 80)
            feats[row_off[b] + t, c] = ((raw[g] + mean[c]).astype(F32) * istd[c]).astype(F32)
        pi = f + 3
        t1, j1 = pi // 6, pi % 6
        if t1 < T:
            emit(t1, j1)
        if j1 == 0 and t1 >= 1:
            emit(t1 - 1, 6)
        if f == 0:
            for j in range(3):
                emit(0, j)
        if f == F - 1:
            for j in range(7):
                if edge(6 * (T - 1) + j, F):
                    emit(T - 1, j)
    return feats


def all_cases():
    return [R.case_tones(), R.case_impulses(16384), R.case_impulses(1), R.case_extremes(), R.case_counts(), R.case_counts_130(),
            R.case_single_frame(), R.case_single_frame_among_empty()]


def fused_cases():
    return [R.case_counts(), R.case_counts_130(), R.case_single_frame(), R.case_single_frame_among_empty()]


def worst_factor(defect):
    """The largest error over bound the GPU tests' comparison reports for the restatement with this defect, over every fbank case
    (inf where a check that allows no error, the floor or a bit-for-bit comparison, fails)."""
    worst = 0.0
    mean, istd = R.cmvn_vectors()
    for case in all_cases():
        raw = sim_raw(case, defect)
        r_max, r_med, bad_floor = R.fbank_ratios(raw, case)
        worst = max(worst, r_max, r_med, np.inf if bad_floor else 0.0)
    for case in fused_cases():
        row_off, rows = R.fused_layout(case)
        raw = sim_raw(case, 0)                       # the scatter is judged on its own: against the same launch's raw frames
        feats = sim_fused(case, raw, row_off, rows, mean, istd, defect if defect in (7, 9) else 0)
        if R.fused_mismatches(feats, raw, case, row_off, mean, istd, CANARY):
            worst = np.inf
    return worst


def test_restatement_of_the_kernel_passes():
    """With no defect the numpy restatement of the kernel passes every fbank case's comparison, and its fused form equals LfrCmvn of
    its raw frames bit for bit, canary rows included."""
    mean, istd = R.cmvn_vectors()
    for case in all_cases():
        R.check_fbank(sim_raw(case), case)
    for case in fused_cases():
        row_off, rows = R.fused_layout(case)
        raw = sim_raw(case)
        assert R.fused_mismatches(sim_fused(case, raw, row_off, rows, mean, istd), raw, case, row_off, mean, istd, CANARY) == 0


@pytest.mark.parametrize("defect", [1, 2, 3, 4, 5, 6, 8, 9])
def test_seeded_defect_is_caught(defect):
    """Each seeded defect fails at least one fbank case by 10 times its bound or more.  The project's "mutation check, not run on the
    GPU" of the BLSTM pin, as a test.  Largest error over bound reached, measured on the CPU:
      1 last mel tap dropped            6.6e3           5 partner at k                    1.0e6
      2 neighbour from the same n1      inf             6 mean / 512                      inf
      3 d[0] for sample 0               1.2e5           8 lookup after an empty utterance 6.7e4
      4 no twiddle sign flip            6.3e5           9 right edge `> F + 3`            inf
    (inf: a comparison that allows no error failed — the floor elements of the constant inputs, or the bit-for-bit fused form.)"""
    factor = worst_factor(defect)
    print(f"defect {defect}: worst error over bound {factor:.3g}")
    assert factor >= 10.0, (defect, factor)


def test_right_edge_mutant_is_equivalent():
    """Defect 7, the right-edge replicate condition `> F + 2` written `>= F + 2`, cannot be caught by any test: padded index F + 2 IS
    the last frame (frame f sits at padded index f + 3), so the extra slot the mutant emits is the slot the last frame's own emit
    writes, with the same value.  Asserted here for F = 1 .. 199 (bit-identical output), so that the claim is checked and not
    assumed; the nearest mutant that does change the output (`> F + 3`, defect 9) is in test_seeded_defect_is_caught."""
    mean, istd = R.cmvn_vectors()
    rng = np.random.default_rng(7)

    class Layout:
        pass
    for F in range(1, 200):
        c = Layout()
        c.nframes, c.frame_off, c.total = [F], [0, F], F
        raw = rng.standard_normal((F, 80)).astype(F32)
        rows = (F + 5) // 6 + 2
        a = sim_fused(c, raw, [0], rows, mean, istd, 0)
        b = sim_fused(c, raw, [0], rows, mean, istd, 7)
        assert np.array_equal(a, b), F
        assert R.fused_mismatches(a, raw, c, [0], mean, istd, CANARY) == 0, F
