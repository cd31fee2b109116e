"""The LayerNorm-folded GEMMs and their row statistics against an fp64 LayerNorm (csrc/gemm_p3.hip, gemm_x3.hip, gemm_x6.hip).

On large batches no LayerNorm kernel runs: the producer GEMM leaves (mean, M2) per row and 128-column tile (`stats_out`), the
consumer applies rstd_i * (x W'^T - mean_i * colsum) + bias' in its epilogue (`ln_stats` / `ln_tiles` / `ln_colsum`) on operands
folded by ops.fold_layernorm.  Reference everywhere: LayerNorm_fp64(A; gamma, beta, eps = 1e-12) @ W^T + bias (+ R1) (ReLU) with
random gamma and beta, computed from the UNFOLDED fp32 weights in NumPy fp64.

Bound of the value tests: the project's GEMM bound 3e-5 * max(1, sqrt(K / 512)) (test_gpu_ops.py::test_gemm_on_pre_split_operands),
plane output + 2^-21 max|ref| (the two planes' own rounding)."""
import contextlib
import importlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

EPS = 1e-12
RATIOS = (0, 1, 4, 16, 64, 256, 1024, 4096)          # mean / std of a row group of the stated-domain sweep
SCALES = (2.0 ** -6, 1.0, 2.0 ** 8)                  # its row scale


@pytest.fixture(scope="module")
def ops_cpu(pkg):
    return importlib.import_module("asr_2pass_amd.ops")


@pytest.fixture(scope="module")
def ops(ops_cpu):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return ops_cpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rup(v, m=128):
    return (v + m - 1) // m * m


def pad_rows(a, rows):
    out = np.zeros((rows,) + a.shape[1:], a.dtype)
    out[:a.shape[0]] = a
    return out


def bound(K):
    return 3e-5 * max(1.0, np.sqrt(K / 512))


def ln64(A, g, b):
    A = A.astype(np.float64)
    mu = A.mean(1, keepdims=True)
    var = ((A - mu) ** 2).mean(1, keepdims=True)
    return (A - mu) / np.sqrt(var + EPS) * g.astype(np.float64) + b.astype(np.float64)


def tile_stats64(X):
    """[M, T * 128] -> [M, T, 2] fp64: (mean, sum of squared deviations from it) of every 128-column tile."""
    t = X.astype(np.float64).reshape(X.shape[0], -1, 128)
    m = t.mean(2)
    return np.stack([m, ((t - m[..., None]) ** 2).sum(2)], 2)


def stats_dev(X, rows):
    return dev(pad_rows(tile_stats64(X).astype(np.float32), rows))


def layer(ops, rng, N, K, ln=True):
    """A Linear behind a LayerNorm: unfolded fp32 (W, bias, gamma, beta) and what ops.fold_layernorm makes of them."""
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    g = rng.uniform(0.5, 1.5, K).astype(np.float32) * np.where(rng.random(K) < 0.1, -1, 1).astype(np.float32)
    b = (0.5 * rng.standard_normal(K)).astype(np.float32)
    d = dict(W=W, bias=bias, g=g, b=b)
    if ln:
        Wf, bf, cs = ops.fold_layernorm(*(torch.from_numpy(v) for v in (W, bias, g, b)))
        d.update(Wf=Wf.numpy(), bf=bf.numpy(), cs=cs.numpy())
    return d


def ref_fold(A, L, R1=None, relu=False):
    y = ln64(A, L["g"], L["b"]) @ L["W"].astype(np.float64).T + L["bias"].astype(np.float64)
    if R1 is not None:
        y = y + R1.astype(np.float64)
    return np.maximum(y, 0) if relu else y


@contextlib.contextmanager
def launch_ctx(ops, flag=None, exact=False):
    ops.set_launch_ctx(flag, exact)
    try:
        yield
    finally:
        torch.cuda.synchronize()
        ops.set_launch_ctx()


def p3_variants():
    return ((0, None), (64, None), (128, "0"), (256, None), (128, "1"))      # (tile_rows, PFHIP_P3_R3)


def set_r3(monkeypatch, r3):
    if r3 is None:
        monkeypatch.delenv("PFHIP_P3_R3", raising=False)
    else:
        monkeypatch.setenv("PFHIP_P3_R3", r3)


# ---- (f) the algebra, without a GPU ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", [(512, 512), (2048, 384)])
def test_fold_algebra_in_fp64_equals_the_unfused_layernorm(ops_cpu, K, N):
    """ops.fold_layernorm + the epilogue formula rstd * (x W'^T - mean * colsum) + bias', evaluated in fp64, against LayerNorm ->
    Linear in fp64 on zero-mean unit-variance rows.  W' and bias' are rounded to fp32 once by fold_layernorm (as the library does at
    load): relative 2^-24 per weight, i.e. at most 2^-24 * sum_k |x^_k W'_nk| <= 6e-8 * sqrt(K) * ~1.2 = 3e-6 at K = 2048 against the
    unrounded fold; with that rounding taken out (the fold redone in fp64) only fp64 rounding is left: 1e-12."""
    rng = np.random.default_rng(K + N)
    A = rng.standard_normal((300, K)).astype(np.float32)
    L = layer(ops_cpu, rng, N, K)
    ref = ref_fold(A, L)
    A64 = A.astype(np.float64)
    mean = A64.mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(((A64 - mean) ** 2).mean(1, keepdims=True) + EPS)
    W64, g64, b64 = L["W"].astype(np.float64), L["g"].astype(np.float64), L["b"].astype(np.float64)
    Wf64 = W64 * g64[None, :]
    exact = rstd * (A64 @ Wf64.T - mean * Wf64.sum(1)[None, :]) + (L["bias"].astype(np.float64) + W64 @ b64)
    assert np.abs(exact - ref).max() < 1e-12
    # what fold_layernorm returns: the same three arrays, each within fp32 rounding of the fp64 ones, colsum taken from the ROUNDED W'
    assert np.abs(L["Wf"] - Wf64).max() <= 2.0 ** -24 * np.abs(Wf64).max()
    bf64, cs64 = L["bias"].astype(np.float64) + W64 @ b64, L["Wf"].astype(np.float64).sum(1)
    assert np.abs(L["bf"] - bf64).max() <= 2.0 ** -24 * np.abs(bf64).max()
    assert np.abs(L["cs"] - cs64).max() <= 2.0 ** -24 * np.abs(cs64).max()
    folded = rstd * (A64 @ L["Wf"].astype(np.float64).T - mean * L["cs"].astype(np.float64)[None, :]) + L["bf"].astype(np.float64)
    assert np.abs(folded - ref).max() < 4e-6


# ---- (a) value of the fold, plane-image operands ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("K,N", [(512, 512), (512, 1536), (2048, 512), (2048, 1536)])
def test_fold_on_plane_operands_matches_fp64_layernorm(ops, monkeypatch, K, N):
    """gemm_p3.hip with ln_stats: every tile height, the three-stage ring, ln_tiles = 4 (K = 512) and 16 (K = 2048, the decoder's form),
    ragged M; fp32 output (+R1), plane output (ReLU, FFN1's form) and the QKV form (fp32 Q | row-major K, V planes)."""
    rng = np.random.default_rng(1000 + K + N)
    L = layer(ops, rng, N, K)
    ws = ops.best_w_scale(float(np.abs(L["Wf"]).max()))
    w_img = ops.split_planes(dev(L["Wf"]), scale=ws)
    bf, cs = dev(L["bf"]), dev(L["cs"])
    tol = bound(K)
    for M in (1, 127, 129, 777, 2050):
        Mp = rup(M)
        A = rng.standard_normal((M, K)).astype(np.float32)
        R1 = rng.standard_normal((M, N)).astype(np.float32)
        a_img = ops.split_planes(dev(A))
        kw = dict(w_scale=ws, bias=bf, ln_stats=stats_dev(A, Mp), ln_tiles=K // 128, ln_colsum=cs)
        ref = ref_fold(A, L, R1)
        ref_relu = ref_fold(A, L, relu=True)
        dR1 = dev(pad_rows(R1, Mp))
        for tr, r3 in p3_variants():
            set_r3(monkeypatch, r3)
            C, P = ops.gemm_p3(a_img, w_img, M, N, K, R1=dR1, want_c=True, want_planes=True, tile_rows=tr, **kw)
            err = np.abs(C.cpu().numpy()[:M] - ref).max()
            errp = np.abs(ops.planes_to_float(P[0], P[1], P[2], N)[:M] - ref).max()
            _, P2 = ops.gemm_p3(a_img, w_img, M, N, K, relu=True, want_c=False, want_planes=True, tile_rows=tr, **kw)
            errr = np.abs(ops.planes_to_float(P2[0], P2[1], P2[2], N)[:M] - ref_relu).max()
            print(f"p3 fold K={K} N={N} M={M} tile={tr} r3={r3}: C {err:.2e} planes {errp:.2e} relu planes {errr:.2e} (bound {tol:.1e})")
            assert err < tol, (M, tr, r3, err)
            assert errp < tol + 2.0 ** -21 * np.abs(ref).max(), (M, tr, r3, errp)
            assert errr < tol + 2.0 ** -21 * np.abs(ref_relu).max(), (M, tr, r3, errr)
        set_r3(monkeypatch, None)
        if N == 1536:
            ref_q = ref_fold(A, L)
            for tr in (0, 64, 128):
                Cq, (kvh, kvl) = ops.gemm_p3_qkv(a_img, w_img, M, N, K, 512, tile_rows=tr, **kw)
                errq = np.abs(Cq.cpu().numpy()[:M] - ref_q[:, :512]).max()
                kv = kvh.cpu().numpy()[:M].astype(np.float64) + kvl.cpu().numpy()[:M].astype(np.float64)
                errkv = np.abs(kv - ref_q[:, 512:]).max()
                print(f"p3 qkv fold K={K} M={M} tile={tr}: Q {errq:.2e} KV planes {errkv:.2e}")
                assert errq < tol, (M, tr, errq)
                assert errkv < tol + 2.0 ** -21 * np.abs(ref_q).max(), (M, tr, errkv)


# ---- (b) the same for the in-loop-split forms ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("K,N", [(512, 512), (512, 1536), (2048, 512)])
def test_fold_on_fp32_operands_matches_fp64_layernorm(ops, K, N, exact):
    """launch_gemm (GemmKernel::SplitBySize) through pfhip_op_gemm_f32_ln: gemm_x3.hip (default) and gemm_x6.hip (exact).  Row counts on both sides
    of gemm_x6_ln_ok (1408 rows = 11 row panels: off; 1409: on), of the 64- / 128-row tile switch (128 tiles of 128 x 128) and ragged."""
    rng = np.random.default_rng(2000 + K + N)
    L = layer(ops, rng, N, K)
    Wf, bf, cs = dev(pad_rows(L["Wf"], rup(N))), dev(L["bf"]), dev(L["cs"])
    ws = ops.best_w_scale(float(np.abs(L["Wf"]).max()))
    tol = bound(K)
    for M in (1, 129, 1408, 1409, 4200):
        Mp = rup(M)
        A = rng.standard_normal((M, K)).astype(np.float32)
        R1 = rng.standard_normal((M, N)).astype(np.float32)
        with launch_ctx(ops, exact=exact):
            C = ops.gemm_f32_ln(dev(pad_rows(A, Mp)), Wf, M=M, N=N, bias=bf, R1=dev(pad_rows(R1, Mp)), ln_stats=stats_dev(A, Mp),
                                ln_tiles=K // 128, ln_colsum=cs, w_scale=ws).cpu().numpy()
            C2 = ops.gemm_f32_ln(dev(pad_rows(A, Mp)), Wf, M=M, N=N, bias=bf, relu=True, ln_stats=stats_dev(A, Mp), ln_tiles=K // 128,
                                 ln_colsum=cs, w_scale=ws).cpu().numpy()
        err = np.abs(C[:M] - ref_fold(A, L, R1)).max()
        err2 = np.abs(C2[:M] - ref_fold(A, L, relu=True)).max()
        print(f"{'x6' if exact else 'x3'} fold K={K} N={N} M={M}: {err:.2e} relu {err2:.2e} (bound {tol:.1e})")
        assert err < tol and err2 < tol, (M, err, err2)


# ---- (c) stats_out against fp64 --------------------------------------------------------------------------------------------------
def check_stats(st, ref, M, K, what):
    """st [rows, T, 2] fp32 from the kernel, ref [M, N] the fp64 result row (bias, residual, ReLU applied).

    Tolerance, from the GEMM bound b = bound(K) alone: the kernel's tile values are y^_j = y_j + e_j with |e_j| <= b.
      mean:  |mean^ - mean| <= b, plus the fp32 rounding of a 128-term sum (<= 8 roundings of 2^-24 relative to the partial sums):
             2^-20 max|y|.
      M2:    with d_j = y_j - mean (sum d_j = 0):  M2^ = sum (d_j + e_j - e_mean)^2 = M2 + 2 sum d_j e_j + sum (e_j - e_mean)^2, and
             |2 sum d_j e_j| <= 2 sqrt(sum d_j^2) sqrt(sum e_j^2) <= 2 sqrt(128 M2) b,   sum (e_j - e_mean)^2 <= 128 b^2;
             fp32 rounding of the squares and of their 128-term sum: 2^-20 M2.
    Rows >= M must not be written (the buffer is pre-filled with a sentinel)."""
    b = bound(K)
    want = tile_stats64(ref)
    got = st[:M].astype(np.float64)
    t = ref.reshape(M, -1, 128)
    e_mean = np.abs(got[..., 0] - want[..., 0]) - (b + 2.0 ** -20 * np.abs(t).max(2))
    tol_m2 = 2 * np.sqrt(128 * want[..., 1]) * b + 128 * b * b + 2.0 ** -20 * want[..., 1]
    e_m2 = np.abs(got[..., 1] - want[..., 1]) - tol_m2
    print(f"stats {what}: mean err {np.abs(got[..., 0] - want[..., 0]).max():.2e} (b {b:.1e}), "
          f"M2 err / tol {(np.abs(got[..., 1] - want[..., 1]) / tol_m2).max():.3f}")
    assert e_mean.max() < 0, (what, e_mean.max())
    assert e_m2.max() < 0, (what, e_m2.max())
    assert (st[M:] == -7.0).all(), what


@gpu
@pytest.mark.parametrize("K,N", [(512, 512), (512, 2048), (2048, 512)])
def test_row_statistics_match_fp64(ops, monkeypatch, K, N):
    """stats_out of the producer form (+bias, +R1; N = 512: four tiles, N = 2048: the decoder's sixteen) on every gemm_p3 tile and on
    the in-loop-split forms, and of a launch that folds a LayerNorm and applies ReLU at the same time."""
    rng = np.random.default_rng(3000 + K + N)
    L = layer(ops, rng, N, K)
    ws = ops.best_w_scale(float(np.abs(L["W"]).max()))
    wsf = ops.best_w_scale(float(np.abs(L["Wf"]).max()))
    w_img, wf_img = ops.split_planes(dev(L["W"]), scale=ws), ops.split_planes(dev(L["Wf"]), scale=wsf)
    for M in (1, 127, 129, 777, 2050):
        Mp = rup(M)
        A = rng.standard_normal((M, K)).astype(np.float32)
        R1 = (rng.standard_normal((M, N)) + 0.5).astype(np.float32)
        ref = A.astype(np.float64) @ L["W"].astype(np.float64).T + L["bias"] + R1
        ref_ln = ref_fold(A, L, relu=True)
        a_img, dR1 = ops.split_planes(dev(A)), dev(pad_rows(R1, Mp))
        lnkw = dict(ln_stats=stats_dev(A, Mp), ln_tiles=K // 128, ln_colsum=dev(L["cs"]))
        for tr, r3 in p3_variants():
            set_r3(monkeypatch, r3)
            st = torch.full((Mp, N // 128, 2), -7.0, device="cuda")
            ops.gemm_p3(a_img, w_img, M, N, K, w_scale=ws, bias=dev(L["bias"]), R1=dR1, want_c=True, want_planes=True, stats_out=st, tile_rows=tr)
            check_stats(st.cpu().numpy(), ref, M, K, f"p3 K={K} N={N} M={M} tile={tr} r3={r3}")
            st = torch.full((Mp, N // 128, 2), -7.0, device="cuda")
            ops.gemm_p3(a_img, wf_img, M, N, K, w_scale=wsf, bias=dev(L["bf"]), relu=True, want_c=True, want_planes=True, stats_out=st,
                        tile_rows=tr, **lnkw)
            check_stats(st.cpu().numpy(), ref_ln, M, K, f"p3 ln+relu K={K} N={N} M={M} tile={tr} r3={r3}")
        set_r3(monkeypatch, None)
        with pytest.raises(ops.PfhipError):          # the statistics come out of the fp32 epilogue: planes alone cannot leave them
            ops.gemm_p3(a_img, w_img, M, N, K, w_scale=ws, want_c=False, want_planes=True, stats_out=st)
        for exact in (False, True):
            with launch_ctx(ops, exact=exact):
                st = torch.full((Mp, N // 128, 2), -7.0, device="cuda")
                ops.gemm_f32_ln(dev(pad_rows(A, Mp)), dev(L["W"]), M=M, N=N, bias=dev(L["bias"]), R1=dR1, stats_out=st, w_scale=ws)
                st2 = torch.full((Mp, N // 128, 2), -7.0, device="cuda")
                ops.gemm_f32_ln(dev(pad_rows(A, Mp)), dev(L["Wf"]), M=M, N=N, bias=dev(L["bf"]), relu=True, stats_out=st2, w_scale=wsf, **lnkw)
            check_stats(st.cpu().numpy(), ref, M, K, f"{'x6' if exact else 'x3'} K={K} N={N} M={M}")
            check_stats(st2.cpu().numpy(), ref_ln, M, K, f"{'x6' if exact else 'x3'} ln+relu K={K} N={N} M={M}")


# ---- (d) producer -> consumer ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("form", ["p3", "x3", "x6"])
@pytest.mark.parametrize("d1,d2", [(512, 2048), (2048, 512)])
def test_statistics_hand_off_through_three_gemms(ops, form, d1, d2):
    """The encoder / decoder hand-off as the model launches it:
        GEMM 1  x1 = x0 W1^T + b1 + R       [M, d1], leaves stats_out (d1 / 128 tiles: 4, or the decoder's 16)
        GEMM 2  h  = ReLU(LN(x1) W2^T + b2) [M, d2], folded, fed x1 (planes, or its fp32 C) AND GEMM 1's own statistics; planes out
        GEMM 3  y  = h W3^T + b3 + R3       [M, 512], stats_out again
    b1 carries a common offset of 1 (rows of x1 have mean / std ~ 0.7: the mean * colsum term is of the size of the result).

    Stage bounds: every GEMM is checked against fp64 of ITS OWN actual inputs at the project bound (planes + 2^-21 max).  The end is
    checked against the fp64 three-step reference with the stage bounds b1, b2, b3 propagated to first order; an elementwise error
    of size <= b with independent signs across k passes a row w of the next Linear as at most 4 sigma = 4 b ||w||_2 (the project
    bound's own sqrt(K) law is the same argument), LayerNorm scales it by rstd:
        tol = b3 + 4 max||W3_n|| (b2 + 2^-21 max|h| + 4 max(rstd) max||W2'_n|| b1)
    Statistics from stats_out and statistics computed on the host in fp64 from the same x1 must give h within b2 of each other."""
    rng = np.random.default_rng(4000 + d1 + d2 + len(form))
    M, d0 = 1500, 512
    Mp = rup(M)
    L1, L2, L3 = layer(ops, rng, d1, d0, ln=False), layer(ops, rng, d2, d1), layer(ops, rng, 512, d2, ln=False)
    L1["bias"] = (L1["bias"] + 1.0).astype(np.float32)
    x0 = rng.standard_normal((M, d0)).astype(np.float32)
    R = rng.standard_normal((M, d1)).astype(np.float32)
    R3 = rng.standard_normal((M, 512)).astype(np.float32)
    f64 = lambda a: a.astype(np.float64)
    b1, b2, b3 = bound(d0), bound(d1), bound(d2)
    ws = [ops.best_w_scale(float(np.abs(w).max())) for w in (L1["W"], L2["Wf"], L3["W"])]
    st1 = torch.full((Mp, d1 // 128, 2), -7.0, device="cuda")
    st3 = torch.full((Mp, 4, 2), -7.0, device="cuda")
    dR, dR3, cs = dev(pad_rows(R, Mp)), dev(pad_rows(R3, Mp)), dev(L2["cs"])

    def stage2(stats):
        if form == "p3":
            _, P = ops.gemm_p3(x1_img, w2, M, d2, d1, w_scale=ws[1], bias=dev(L2["bf"]), relu=True, want_c=False, want_planes=True,
                               ln_stats=stats, ln_tiles=d1 // 128, ln_colsum=cs)
            return P, ops.planes_to_float(P[0], P[1], P[2], d2)[:M]
        with launch_ctx(ops, exact=form == "x6"):
            h = ops.gemm_f32_ln(x1_dev, dev(L2["Wf"]), M=M, N=d2, bias=dev(L2["bf"]), relu=True, ln_stats=stats, ln_tiles=d1 // 128,
                                ln_colsum=cs, w_scale=ws[1])
        return h, f64(h.cpu().numpy()[:M])

    if form == "p3":
        w1, w2, w3 = (ops.split_planes(dev(w), scale=s) for w, s in zip((L1["W"], L2["Wf"], L3["W"]), ws))
        x1_dev, x1_img = ops.gemm_p3(ops.split_planes(dev(x0)), w1, M, d1, d0, w_scale=ws[0], bias=dev(L1["bias"]), R1=dR, want_c=True,
                                     want_planes=True, stats_out=st1)
        x1 = f64(x1_dev.cpu().numpy()[:M])
        x1_in = ops.planes_to_float(x1_img[0], x1_img[1], x1_img[2], d1)[:M]          # what GEMM 2 multiplies
        h_dev, h = stage2(st1)
        y_dev, _ = ops.gemm_p3(h_dev, w3, M, 512, d2, w_scale=ws[2], bias=dev(L3["bias"]), R1=dR3, want_c=True, stats_out=st3)
    else:
        with launch_ctx(ops, exact=form == "x6"):
            x1_dev = ops.gemm_f32_ln(dev(pad_rows(x0, Mp)), dev(L1["W"]), M=M, N=d1, bias=dev(L1["bias"]), R1=dR, stats_out=st1, w_scale=ws[0])
        x1 = x1_in = f64(x1_dev.cpu().numpy()[:M])
        h_dev, h = stage2(st1)
        with launch_ctx(ops, exact=form == "x6"):
            y_dev = ops.gemm_f32_ln(h_dev, dev(L3["W"]), M=M, N=512, bias=dev(L3["bias"]), R1=dR3, stats_out=st3, w_scale=ws[2])
    y = f64(y_dev.cpu().numpy()[:M])
    # stage by stage, each against fp64 of its own actual inputs
    r1 = f64(x0) @ f64(L1["W"]).T + L1["bias"] + R
    check_stats(st1.cpu().numpy(), r1, M, d0, f"{form} hand-off stage 1")
    r2_own = ref_fold(x1_in.astype(np.float64), L2, relu=True)
    r3_own = h @ f64(L3["W"]).T + L3["bias"] + R3
    e1, e2, e3 = np.abs(x1 - r1).max(), np.abs(h - r2_own).max(), np.abs(y - r3_own).max()
    # the end against the three-step fp64 reference
    r2 = ref_fold(r1, L2, relu=True)
    r3 = r2 @ f64(L3["W"]).T + L3["bias"] + R3
    rstd = 1.0 / np.sqrt(r1.var(1) + EPS)
    n2 = lambda w: np.sqrt((f64(w) ** 2).sum(1)).max()
    tol = b3 + 4 * n2(L3["W"]) * (b2 + 2.0 ** -21 * np.abs(r2).max() + 4 * rstd.max() * n2(L2["Wf"]) * b1)
    e_end = np.abs(y - r3).max()
    # host statistics of the same x1 against the kernel's own
    _, h_host = stage2(stats_dev(x1_in, Mp))
    e_st = np.abs(h_host - h).max()
    print(f"hand-off {form} {d1}->{d2}: stage errors {e1:.2e} {e2:.2e} {e3:.2e} (bounds {b1:.1e} {b2:.1e} {b3:.1e}), end {e_end:.2e} "
          f"(tol {tol:.2e}), host vs kernel statistics {e_st:.2e}")
    assert e1 < b1 and e2 < b2 + (2.0 ** -21 * np.abs(r2_own).max() if form == "p3" else 0.0) and e3 < b3, (e1, e2, e3)
    assert e_end < tol, (e_end, tol)
    assert e_st < b2, e_st
    check_stats(st3.cpu().numpy(), r3_own, M, d2, f"{form} hand-off stage 3")


# ---- (e) stated domain of the fold -----------------------------------------------------------------------------------------------
def fold_domain_sweep(ops, form, rows=128, seed=5):
    """One launch per row group (rows x 512, mean / std = r, scale s) with a fresh range flag.  Returns records with the max error
    against fp64 (inf when an output is not finite), the error E32 of the fp32 restatement of the UNFOLDED path (LayerNorm in fp32,
    then an fp32 matmul: what the reference's plain-fp32 graph does) and the flag."""
    K = N = 512
    rng = np.random.default_rng(seed)
    L = layer(ops, rng, N, K)
    ws = ops.best_w_scale(float(np.abs(L["Wf"]).max()))
    Wf, bf, cs = dev(L["Wf"]), dev(L["bf"]), dev(L["cs"])
    w_img = ops.split_planes(Wf, scale=ws)
    rp = rup(rows)
    out = []
    for s in SCALES:
        for r in RATIOS:
            A = ((rng.standard_normal((rows, K)) + r) * s).astype(np.float32)
            ref = ref_fold(A, L)
            a32 = A - A.mean(1, keepdims=True, dtype=np.float32)
            var32 = (a32 * a32).mean(1, keepdims=True, dtype=np.float32)
            y32 = (a32 / np.sqrt(var32 + np.float32(EPS)) * L["g"] + L["b"]).astype(np.float32) @ L["W"].T + L["bias"]
            e32 = float(np.abs(y32.astype(np.float64) - ref).max())
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            st = stats_dev(A, rp)
            with launch_ctx(ops, flag=flag, exact=form in ("x6", "exact")):
                if form == "exact":          # what a flagged forward is redone on: the LayerNorm kernel, then the bf16 three-plane GEMM
                    y = ops.layernorm(dev(pad_rows(A, rp)), dev(L["g"]), dev(L["b"]))
                    C = ops.gemm_f32_ln(y, dev(L["W"]), M=rows, N=N, bias=dev(L["bias"]), w_scale=ops.best_w_scale(float(np.abs(L["W"]).max())))
                elif form == "p3":
                    C, _ = ops.gemm_p3(ops.split_planes(dev(A)), w_img, rows, N, K, w_scale=ws, bias=bf, ln_stats=st, ln_tiles=4, ln_colsum=cs)
                else:
                    C = ops.gemm_f32_ln(dev(pad_rows(A, rp)), Wf, M=rows, N=N, bias=bf, ln_stats=st, ln_tiles=4, ln_colsum=cs, w_scale=ws)
                C = C.cpu().numpy()[:rows]
            err = float(np.abs(C - ref).max()) if np.isfinite(C).all() else float("inf")
            out.append(dict(form=form, rows=rows, r=r, s=s, err=err, e32=e32, flag=int(flag.item())))
    return out


@gpu
@pytest.mark.parametrize("form", ["x3", "p3", "exact"])
def test_fold_stated_domain(ops, form):
    """Where the fold stops being an fp32 LayerNorm -> GEMM, pinned.  x W'^T and mean * colsum are both of size |mean|, their
    difference of size std: the fold loses about mean / std of the accumulation's and the planes' precision, on rows whose every
    element fits fp16 comfortably.  Row groups of 128 with mean / std r times row scale s, one launch and one fresh flag each:
      * r <= 1 at every scale: within the project bound, flag down;
      * every other group: within max(project bound, 4 * E32) (E32 = the fp32 unfolded restatement's error on the same group; 4 =
        the two bits the planes give up against fp32, 2^-22 vs 2^-24) OR the range flag is up;
      * the exact form (what a flagged forward is redone on): max(project bound, 4 * E32) on every group, no excuse.  The fold on the
        bf16 three-plane kernels misses this from r = 16 on as well (5.1e-5 .. 5.3e-5 against 4 * E32 = 2.4e-5 .. 3.1e-5: the
        cancellation happens in the fp32 accumulator), so the exact forward does not fold: LayerNorm kernel + three-plane GEMM.
    Measured values: the table in DESIGN.md section 2; the limit kLnOffsetMax = 4 (csrc/kernels.h) is read off it."""
    b = bound(512)
    bad = []
    for g in fold_domain_sweep(ops, form):
        lim = max(b, 4 * g["e32"])
        print(f"{form} r={g['r']:5d} s=2^{int(np.log2(g['s'])):+d}: err {g['err']:.2e} E32 {g['e32']:.2e} flag {g['flag']}")
        if g["r"] <= 1:
            ok = g["err"] < b and g["flag"] == 0
        elif form == "exact":
            ok = g["err"] < lim
        else:
            ok = g["err"] < lim or g["flag"] != 0
        if not ok:
            bad.append(g)
    assert not bad, bad
