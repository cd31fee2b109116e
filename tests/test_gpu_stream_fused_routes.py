"""GPU: every route of the one-window fused launches (csrc/stream_fused.hip: fused_gemv1t_kernel, fused_ln_gemv_kernel,
fused_ln_gemm_kernel) through the operator entries, one case per route from tests/stream_fused_cases.py, at both ends of the
route's row range.

Each case runs twice:
  exact  (forms without LayerNorm) integer operands — A, W, FSMN rows and taps in [-4, 4], bias / R1 / R2 in [-64, 64] — so that
         |A W^T| <= 16 * 4096 and every partial sum in any order is an integer far below 2^24: exact in fp32 with fmaf or the fp32
         matrix instruction.  Compared with np.array_equal against the integer reference (formed in float64, where the same sums
         are exact below 2^53, and checked on the CPU against the same expression in float32 numpy).  A dropped or doubled k-block,
         a wrong wave count, a wrong row clamp or a mis-indexed epilogue term cannot pass.
  fp64   the data of test_fused_ln_gemm_one_window / test_fused_gemv_one_trip (rows with mean 1.5 / 4.5 and spread 3, gamma in
         [0.5, 1.5], beta ~ 0.2, W ~ N(0, 1/K)) against the explicit two-pass LayerNorm in fp64, with those tests' bounds:
         5e-5 * sqrt(K / 512) for fused_ln_gemm, 1e-4 * sqrt(K / 512) for the one-trip form.  The worst error is printed per case.
Contracts, in the same launches: the output starts as 777 everywhere and must still be 777 in rows >= M and columns >= N; rows >= M
of X, rows >= N of W (readable up to the 128-row padding), of bias / column sums / FSMN taps, everything of R2 and the FSMN value
matrix outside [M, N], and with a LayerNorm of width D < K the columns D.. of X, are NaN and must not reach a stored value (W is 0
for k >= D, as the model pads it); R1 is the output buffer itself, as at every call site of stream.cpp; bias is NULL in one of the
two row counts; R2 is given to fused_ln_gemm; ReLU is on in one run and off in the other; FSMN cases also run at 1, 5, 6 and 20
rows where the route is the same, so that the 11-tap window is cut at both ends.
"""
import importlib
import os

import numpy as np
import pytest

import stream_fused_cases as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 777.0
_f = lambda x: np.asarray(x, np.float32)


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    set_knobs = [k for k in T.KNOBS if k in os.environ]
    if set_knobs:
        pytest.fail(f"{set_knobs} change the dispatch under test: unset them")
    return importlib.import_module("asr_2pass_amd.ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_pools = {}


def _pool(rows, cols):
    """Random operands drawn once and shared by every case (integers in [-4, 4] and standard normals): a case takes a window."""
    big = rows > 768
    shape = (8448 + 64, 640) if big else (768 + 64, 4096)
    assert rows <= shape[0] - 64 and cols <= shape[1], (rows, cols)
    if big not in _pools:
        rng = np.random.default_rng(20261020 + big)
        _pools[big] = (rng.integers(-4, 5, shape).astype(np.float32), rng.standard_normal(shape, dtype=np.float32))
    return _pools[big]


def _operands(c, idx, integer):
    """Everything but X and the row count: W [Np, K] with NaN rows beyond N, bias, FSMN taps, gamma / beta, D."""
    Np = (c.N + 127) // 128 * 128
    rng = np.random.default_rng(1000 * idx + integer)
    pi, pf = _pool(Np, c.K)
    off = (7 * idx) % 64
    W = (pi if integer else pf)[off:off + Np, :c.K].copy()
    if not integer:
        W *= np.float32(1.0 / np.sqrt(c.K))
    W[c.N:] = np.nan
    D = c.K
    if c.form == "ln_gemm" and c.ln:                 # whole k-blocks dead (K - 128), part of one (K - 16), none
        D = [c.K, c.K - 16, c.K - 128 if c.K > 128 else c.K - 16][idx % 3]
        W[:, D:] = 0
    vec = lambda lo_hi, scale: _f(rng.integers(-lo_hi, lo_hi + 1, Np) if integer else rng.standard_normal(Np) * scale)
    bias = vec(64, 1.0); bias[c.N:] = np.nan
    fw = _f(rng.integers(-4, 5, (Np, 11)) if integer else rng.standard_normal((Np, 11)) / 3); fw[c.N:] = np.nan
    g = _f(rng.random(c.K) + 0.5)
    b = _f(rng.standard_normal(c.K) * 0.2)
    return dict(Np=Np, W=W, D=D, bias=bias, fw=fw, g=g, b=b)


def _rows(c, idx, M, Np, D, integer):
    """X [32, K] and the [32, Np] epilogue matrices for M rows, NaN wherever the kernels have no business."""
    rng = np.random.default_rng(100000 + 1000 * idx + 10 * M + integer)
    X = np.full((32, c.K), np.nan, np.float32)
    mats = []
    if integer:
        X[:M, :D] = rng.integers(-4, 5, (M, D))
    else:
        X[:M, :D] = rng.standard_normal((M, D)) * 3 + (4.5 if c.form == "1trip" else 1.5)
    for lim in (64, 64, 4):                          # R1, R2, V
        a = np.full((32, Np), np.nan, np.float32)
        a[:M, :c.N] = rng.integers(-lim, lim + 1, (M, c.N)) if integer else rng.standard_normal((M, c.N))
        mats.append(a)
    return X, mats[0], mats[1], mats[2]


def _reference(c, M, o, X, R1, R2, V, use, dtype):
    """relu(LN?(X) W^T + bias + R1 + R2 + FSMN memory of V) over [M, N] in `dtype` (float64, or float32 for the exactness check)."""
    t = lambda a: a.astype(dtype)
    N, D = c.N, o["D"]
    x = t(X[:M, :D])
    if c.ln:                                         # explicit two-pass LayerNorm
        mean = x.mean(1, keepdims=True)
        var = ((x - mean) ** 2).mean(1, keepdims=True)
        x = (x - mean) / np.sqrt(var + dtype(1e-12)) * t(o["g"][:D]) + t(o["b"][:D])
    ref = x @ t(o["W"][:N, :D]).T
    if use["bias"]:
        ref = ref + t(o["bias"][:N])
    ref = ref + t(R1[:M, :N])
    if use["R2"]:
        ref = ref + t(R2[:M, :N])
    if use["fsmn"]:
        v = t(V[:M, :N])
        mem = v.copy()
        for tt in range(M):
            for j in range(11):
                s = tt + j - 5
                if 0 <= s < M:
                    mem[tt] += t(o["fw"][:N, j]) * v[s]
        ref = ref + mem
    return np.maximum(ref, 0) if use["relu"] else ref


def _launch(ops, c, M, o, dW, X, R1, R2, V, use):
    """One launch with R1 in place; returns the whole [32, Np] output buffer."""
    out = np.full((32, o["Np"]), SENTINEL, np.float32)
    out[:M, :c.N] = R1[:M, :c.N]
    out = dev(out)
    kw = dict(R1=out, fsmn_v=dev(V) if use["fsmn"] else None, fsmn_w=dev(o["fw"]) if use["fsmn"] else None, relu=use["relu"], out=out)
    bias = dev(o["bias"]) if use["bias"] else None
    if c.form == "1trip":
        Wd, cs = dW, None
        if c.ln:                                     # the algebraic LayerNorm's folded weights, as the library builds them at load
            Wd, bias, cs = ops.fold_layernorm(dW, bias, dev(o["g"]), dev(o["b"]))
        ops.fused_gemv_1trip(dev(X), Wd, M, c.N, bias=bias, ln_colsum=cs, **kw)
    else:
        ops.fused_ln_gemm(dev(X), dW, M, c.N, g=dev(o["g"]) if c.ln else None, b=dev(o["b"]) if c.ln else None, D=o["D"], bias=bias,
                          R2=dev(R2) if use["R2"] else None, **kw)
    return out.cpu().numpy()


def _check_untouched(out, M, N, tag):
    assert (out[M:] == SENTINEL).all(), f"{tag}: rows >= M were written"
    assert (out[:, N:] == SENTINEL).all(), f"{tag}: columns >= N were written"


def _case_id(c):
    return c.route if c in T.REPRESENTATIVES else f"{c.route}@{c.N}x{c.K}"


@pytest.mark.parametrize("idx", range(len(T.CASES)), ids=[_case_id(c) for c in T.CASES])
def test_route(ops, idx):
    """Measured on an MI355X, worst fp64 error over the cases of a family as a share of its bound: one-trip form 0.09 (3.0e-6 of
    3.5e-5, FSMN on 8 columns at K = 64), vector form 0.14 (2.5e-6 of 1.8e-5, K = 64), matrix form 0.16 (3.4e-6 of 2.2e-5, K = 96);
    with LayerNorm never above 0.06.  The bounds shrink with sqrt(K) while the epilogue's four or five roundings of values around 8
    do not, so the smallest K sit closest; no route needs more than the bounds of the two older operator tests."""
    c = T.CASES[idx]
    Ms = {c.m_lo, c.m_hi}
    fsmn = c.fsmn or (c.form == "ln_gemm" and idx % 3 == 0)
    if fsmn:
        Ms |= {m for m in (1, 5, 6, 20) if T.route_of(ops, c.form, m, c.N, c.K, c.ln, c.fsmn) == c.route}
    bound = (1e-4 if c.form == "1trip" else 5e-5) * np.sqrt(c.K / 512)
    worst = 0.0
    for integer in ((0,) if c.ln else (1, 0)):
        o = _operands(c, idx, integer)
        dW = dev(o["W"])
        for i, M in enumerate(sorted(Ms)):
            assert T.route_of(ops, c.form, M, c.N, c.K, c.ln, c.fsmn) == c.route
            X, R1, R2, V = _rows(c, idx, M, o["Np"], o["D"], integer)
            use = dict(bias=(i + integer) % 2 == 0, R2=c.form == "ln_gemm" and (integer or i % 2 == 0), fsmn=fsmn,
                       relu=(idx + i + integer) % 2 == 0)
            if c.form == "1trip" and c.ln:
                use["bias"] = True                   # the folded bias exists whether or not the layer has one
            tag = f"{_case_id(c)} M={M} N={c.N} K={c.K} D={o['D']} {'exact' if integer else 'fp64'} {use}"
            ref = _reference(c, M, o, X, R1, R2, V, use, np.float64)
            if integer:
                ref32 = _reference(c, M, o, X, R1, R2, V, use, np.float32)
                assert ref32.dtype == np.float32 and np.array_equal(ref32.astype(np.int64), ref.astype(np.int64)) and \
                    np.array_equal(ref, np.rint(ref)), tag
            out = _launch(ops, c, M, o, dW, X, R1, R2, V, use)
            _check_untouched(out, M, c.N, tag)
            got = out[:M, :c.N]
            if integer:
                bad = got != ref
                assert np.array_equal(got.astype(np.float64), ref) and np.array_equal(got.astype(np.int64), ref.astype(np.int64)), \
                    f"{tag}: {int(bad.sum())} of {bad.size} differ, first at {tuple(np.argwhere(bad)[0])}, worst {np.abs(got - ref).max()}"
            else:
                err = float(np.abs(got - ref).max())
                worst = max(worst, err)
                print(f"fp64 {tag}: max err {err:.3e} (bound {bound:.3e})")
                assert np.isfinite(got).all() and err < bound, tag
    print(f"ROUTE {_case_id(c)} worst fp64 error {worst:.3e} of {bound:.3e}")
