"""The 256 x 256 tile of gemm_p3.hip (one persistent eight-wave workgroup per CU, ring of three 32-KB stages, the C tile out in 32-row
slabs): bit-identical to the 128 x 128 four-stage kernel on both forms it serves (LayerNorm fold with fp32 C: QKV'; with plane images of
C and ReLU: FFN1'), within the two-plane bound of the fp64 product, refused for every other form, and taken by the default dispatch for
the encoder's FFN1' shape."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_case(ops, rng, M, N, K, want_ref=False):
    """Operands in the model's configuration: LayerNorm statistics over 128-column tiles of A as the producer kernels leave them (K a
    multiple of 128: that many tiles), column sums of W, bias."""
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    ws = ops.best_w_scale(float(np.abs(W).max()))
    Mp = (M + 127) // 128 * 128
    if K % 128 == 0:
        T = K // 128
        t = A.reshape(M, T, 128).astype(np.float64)
        stats = np.zeros((Mp, T, 2), np.float32)
        stats[:M, :, 0] = t.mean(2)
        stats[:M, :, 1] = ((t - t.mean(2, keepdims=True)) ** 2).sum(2)
    else:      # a K the statistics' tiling does not divide: any (mean, M2) serve a bit-identity check
        T = 4
        stats = np.zeros((Mp, T, 2), np.float32)
        stats[:M, :, 0] = rng.standard_normal((M, T)) * 0.1
        stats[:M, :, 1] = 128.0 * (0.5 + rng.random((M, T)))
    colsum = W.astype(np.float64).sum(1).astype(np.float32)
    kw = dict(w_scale=ws, bias=dev(bias), ln_stats=dev(stats), ln_tiles=T, ln_colsum=dev(colsum))
    case = dict(a=ops.split_planes(dev(A)), w=ops.split_planes(dev(W), scale=ws), kw=kw, M=M, N=N, K=K)
    if want_ref:
        st = stats[:M].astype(np.float64)
        mean = st[:, :, 0].mean(1)
        var = (st[:, :, 1] + 128.0 * (st[:, :, 0] - mean[:, None]) ** 2).sum(1) / K
        xn = (A.astype(np.float64) - mean[:, None]) / np.sqrt(var[:, None] + 1e-12)
        case["ref"] = xn @ W.astype(np.float64).T + bias
        case["scale"] = max(1.0, float(np.abs(xn).max()))
    return case


def run_forms(ops, c, **sel):
    """(fp32 C of the QKV' form, both plane images of the FFN1' form) as host arrays."""
    M, N, K = c["M"], c["N"], c["K"]
    C, _ = ops.gemm_p3(c["a"], c["w"], M, N, K, want_c=True, want_planes=False, **c["kw"], **sel)
    _, P = ops.gemm_p3(c["a"], c["w"], M, N, K, relu=True, want_c=False, want_planes=True, **c["kw"], **sel)
    torch.cuda.synchronize()
    return C.cpu().numpy()[:M], P[0].cpu().numpy(), P[1].cpu().numpy(), P


def assert_same(ops, c, monkeypatch, tag):
    monkeypatch.setenv("PFHIP_P3_R3", "0")
    ref = run_forms(ops, c, tile_rows=128)
    before = ops.gemm_p3_wide_launches()
    got = run_forms(ops, c, tile_cols=256)
    assert ops.gemm_p3_wide_launches() == before + 2, tag
    assert np.array_equal(got[0], ref[0]), tag
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), tag
    N = c["N"]
    assert np.array_equal(ops.planes_to_float(got[3][0], got[3][1], got[3][2], N), ops.planes_to_float(ref[3][0], ref[3][1], ref[3][2], N)), tag
    return got


MODEL_SHAPES = ((16000, 2048, 512), (16000, 1536, 512))


@pytest.mark.parametrize("M,N,K", MODEL_SHAPES)
def test_wide_tile_is_bit_identical_on_the_model_shapes(ops, monkeypatch, M, N, K):
    """The encoder's FFN1' and QKV' launches of a 32 x 30 s batch (504 / 378 tiles: two per workgroup) and the fp64 bound of
    test_gemm_on_pre_split_operands (3e-5 * max(1, sqrt(K / 512)), scaled like it by nothing else: normalised rows are O(1))."""
    c = make_case(ops, np.random.default_rng(M + N), M, N, K, want_ref=True)
    got = assert_same(ops, c, monkeypatch, (M, N, K))
    tol = 3e-5 * max(1.0, np.sqrt(K / 512))
    err = np.abs(got[0] - c["ref"]).max()
    print(f"fp64 check {M}x{N}x{K}: max abs err {err:.3e} (bound {tol:.1e})")
    assert err < tol
    pl = ops.planes_to_float(got[3][0], got[3][1], got[3][2], N)[:M]
    ref2 = np.maximum(c["ref"], 0)
    err2 = np.abs(pl - ref2).max()
    print(f"fp64 check of the planes: {err2:.3e}")
    assert err2 < tol + 2.0 ** -21 * np.abs(ref2).max()


@pytest.mark.parametrize("M", [1, 255, 257, 777, 1400, 7015])
def test_wide_tile_ragged_rows(ops, monkeypatch, M):
    """Ragged M, among them padded row counts that are odd multiples of 128 (257 -> 384, 1400 -> 1408 = 11 x 128, 7015 -> 7040 = 55 x
    128): the last row panel reaches past the A image and is clamped into it."""
    c = make_case(ops, np.random.default_rng(M), M, 512, 512)
    assert_same(ops, c, monkeypatch, M)


@pytest.mark.parametrize("K", [16, 32, 48, 64, 80, 96, 112, 128, 256, 272, 1040, 2080])
def test_wide_tile_every_tail_of_the_ring(ops, monkeypatch, K):
    """K-steps 1 .. 8 (every phase of the three-stage ring and of the two fragment sets at a tile boundary, the prologue longer than the
    tile included), then long loops.  Every workgroup walks two tiles (five where K <= 48: the DMA cursor then runs up to three tiles
    ahead of the MFMAs), and the tile count does not divide over the grid."""
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    M = 256 * ((4 * cus if K <= 48 else cus) + 3)
    c = make_case(ops, np.random.default_rng(K), M, 256, K)
    assert_same(ops, c, monkeypatch, K)


@pytest.mark.parametrize("N", [256, 512, 768, 1024, 2048])
def test_wide_tile_widths(ops, monkeypatch, N):
    c = make_case(ops, np.random.default_rng(N), 1500, N, 512)
    assert_same(ops, c, monkeypatch, N)


@pytest.mark.parametrize("tiles_per_wg", [1.0, 2.0, 3.0, 1.37, 2.6])
def test_wide_tile_persistent_walk(ops, monkeypatch, tiles_per_wg):
    """One, two and three tiles per workgroup, and tile counts that do not divide over the grid."""
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    tiles = max(1, int(round(cus * tiles_per_wg)))
    tn = 2
    M = 256 * ((tiles + tn - 1) // tn) - 5
    c = make_case(ops, np.random.default_rng(tiles), M, 256 * tn, 128)
    assert_same(ops, c, monkeypatch, tiles)


@pytest.mark.parametrize("M,N,K", MODEL_SHAPES)
def test_wide_tile_race_screen(ops, monkeypatch, M, N, K):
    """The sync structure is new: 20 launches of each form over four rotating operand sets, every result compared bit for bit with the
    128-row kernel's.  A comparison, not a stress loop: a mismatch fails here once."""
    monkeypatch.setenv("PFHIP_P3_R3", "0")
    rng = np.random.default_rng(K + N)
    cases = [make_case(ops, rng, M, N, K) for _ in range(4)]
    refs = [run_forms(ops, c, tile_rows=128)[:3] for c in cases]
    Mp = (M + 127) // 128 * 128
    C = torch.empty((Mp, N), dtype=torch.float32, device="cuda")
    for it in range(20):
        c, ref = cases[it & 3], refs[it & 3]
        C.zero_()
        ops.gemm_p3(c["a"], c["w"], M, N, K, want_c=True, want_planes=False, out=C, tile_cols=256, **c["kw"])
        _, P = ops.gemm_p3(c["a"], c["w"], M, N, K, relu=True, want_c=False, want_planes=True, tile_cols=256, **c["kw"])
        torch.cuda.synchronize()
        assert np.array_equal(C.cpu().numpy()[:M], ref[0]), it
        assert np.array_equal(P[0].cpu().numpy(), ref[1]) and np.array_equal(P[1].cpu().numpy(), ref[2]), it


def test_wide_tile_refuses_what_it_does_not_serve(ops):
    """Unsupported forms, N not a multiple of the tile width, K % 16: RuntimeError, nothing launched."""
    c = make_case(ops, np.random.default_rng(5), 300, 512, 512)
    a, w, kw = c["a"], c["w"], c["kw"]
    no_ln = dict(w_scale=kw["w_scale"], bias=kw["bias"])
    R1 = torch.zeros((384, 512), device="cuda")
    before = ops.gemm_p3_wide_launches()
    with pytest.raises(RuntimeError):
        ops.gemm_p3(a, w, 300, 512, 512, tile_cols=256, **no_ln)                                       # no LayerNorm fold
    with pytest.raises(RuntimeError):
        ops.gemm_p3(a, w, 300, 512, 512, want_c=True, want_planes=True, tile_cols=256, **kw)           # both outputs
    with pytest.raises(RuntimeError):
        ops.gemm_p3(a, w, 300, 512, 512, R1=R1, tile_cols=256, **kw)                                   # residual
    with pytest.raises(RuntimeError):
        ops.gemm_p3(a, w, 300, 512, 512, stats_out=torch.zeros((384, 4, 2), device="cuda"), tile_cols=256, **kw)
    with pytest.raises(RuntimeError):
        ops.gemm_p3(a, w, 300, 384, 512, tile_cols=256, **kw)                                          # N % 256
    with pytest.raises(RuntimeError):
        ops.gemm_p3(a, w, 300, 512, 504, tile_cols=256, **kw)                                          # K % 16
    with pytest.raises(RuntimeError):
        ops.gemm_p3(a, w, 300, 512, 512, tile_rows=128, tile_cols=256, **kw)                           # two selectors
    with pytest.raises(RuntimeError):
        ops.gemm_p3(a, w, 300, 512, 512, tile_cols=128, **kw)                                          # no such width
    torch.cuda.synchronize()
    assert ops.gemm_p3_wide_launches() == before


def test_default_dispatch_takes_the_wide_tile_for_ffn1(ops, monkeypatch):
    """tile_rows = 0 on the encoder's shapes: FFN1' (16000 x 2048 x 512, planes out) runs on the 256 x 256 tile; the out-projection and
    FFN2 forms (residual, statistics out) never do; PFHIP_P3_WIDE=0 opts out."""
    monkeypatch.delenv("PFHIP_P3_WIDE", raising=False)
    c = make_case(ops, np.random.default_rng(9), 16000, 2048, 512)
    n0 = ops.gemm_p3_wide_launches()
    ops.gemm_p3(c["a"], c["w"], 16000, 2048, 512, relu=True, want_c=False, want_planes=True, **c["kw"])
    assert ops.gemm_p3_wide_launches() == n0 + 1
    monkeypatch.setenv("PFHIP_P3_WIDE", "0")
    ops.gemm_p3(c["a"], c["w"], 16000, 2048, 512, relu=True, want_c=False, want_planes=True, **c["kw"])
    assert ops.gemm_p3_wide_launches() == n0 + 1
    monkeypatch.delenv("PFHIP_P3_WIDE")
    st = torch.zeros((16000, 16, 2), device="cuda")
    ops.gemm_p3(c["a"], c["w"], 16000, 2048, 512, w_scale=c["kw"]["w_scale"], bias=c["kw"]["bias"], want_c=True, want_planes=True, stats_out=st)
    small = make_case(ops, np.random.default_rng(10), 3000, 2048, 512)      # below the fill rule: the 128-column kernels
    ops.gemm_p3(small["a"], small["w"], 3000, 2048, 512, relu=True, want_c=False, want_planes=True, **small["kw"])
    torch.cuda.synchronize()
    assert ops.gemm_p3_wide_launches() == n0 + 1
