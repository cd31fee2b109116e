"""GPU: the attention forms for head width d_k = 80 (the small Paraformer: d_model 320, four heads) against softmax(QK^T)V in fp64,
through the operator-level C ABI (include/pfhip_ops.h).

  pfhip_op_attention_hd(head_dim = 80)   more than 64 queries in the longest segment: attention_h80.hip (two fp16 planes, three
                                         products on v_mfma_f32_32x32x16_f16, V^T padded to 96 rows in LDS); up to 64 queries, or the
                                         launch context set to exact: the fp32-MFMA attention_kernel<80, false> of attention.hip
  pfhip_op_window_attention_hd(80)       one streaming window, stream_fused.hip window_attention_kernel<80>

Tolerances are the ones tests/test_gpu_ops.py holds the d_k = 128 forms to (2e-5; 3e-4 for scores of magnitude ~500)."""
import contextlib
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H, DK = 4, 80
SELF_LENS = [1, 31, 32, 33, 64, 65, 257, 300]      # a single key, tile edges both sides of 32 and 64, the kernel switch at 64 queries, two query blocks


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def mha64(q, k, v, n_head, dk):
    q, k, v = (a.astype(np.float64) for a in (q, k, v))
    out = np.empty((q.shape[0], n_head * dk))
    for h in range(n_head):
        sl = slice(h * dk, (h + 1) * dk)
        s = q[:, sl] @ k[:, sl].T * dk ** -0.5
        p = np.exp(s - s.max(1, keepdims=True))
        out[:, sl] = (p / p.sum(1, keepdims=True)) @ v[:, sl]
    return out


@contextlib.contextmanager
def exact_ctx(ops):
    ops.set_launch_ctx(None, True)
    try:
        yield
    finally:
        torch.cuda.synchronize()
        ops.set_launch_ctx()


def ragged_case(ops, q_lens, kv_lens, seed, tol=2e-5):
    rng = np.random.default_rng(seed)
    q_off = np.concatenate([[0], np.cumsum(q_lens)[:-1]]).astype(np.int32)
    kv_off = np.concatenate([[0], np.cumsum(kv_lens)[:-1]]).astype(np.int32)
    Q = rng.standard_normal((sum(q_lens), H * DK)).astype(np.float32)
    K = rng.standard_normal((sum(kv_lens), H * DK)).astype(np.float32)
    V = rng.standard_normal((sum(kv_lens), H * DK)).astype(np.float32)
    O = ops.attention(dev(Q), dev(K), dev(V), dev(q_off), dev(np.asarray(q_lens, np.int32)), dev(kv_off),
                      dev(np.asarray(kv_lens, np.int32)), H, DK ** -0.5, head_dim=DK).cpu().numpy()
    assert O.shape == (sum(q_lens), H * DK) and np.isfinite(O).all()
    worst = 0.0
    for b in range(len(q_lens)):
        ref = mha64(Q[q_off[b]:q_off[b] + q_lens[b]], K[kv_off[b]:kv_off[b] + kv_lens[b]], V[kv_off[b]:kv_off[b] + kv_lens[b]], H, DK)
        err = float(np.abs(O[q_off[b]:q_off[b] + q_lens[b]] - ref).max())
        print(f"d_k 80 attention: segment {b} ({q_lens[b]} x {kv_lens[b]}) max abs err {err:.3e}")
        worst = max(worst, err)
    assert worst < tol, worst


def test_self_attention_ragged(ops):
    ragged_case(ops, SELF_LENS, SELF_LENS, 80)


def test_self_attention_ragged_short_launch(ops):
    """The same segments up to 64 rows only: the whole launch stays on the fp32-MFMA kernel (no segment above the switch)."""
    lens = [n for n in SELF_LENS if n <= 64]
    ragged_case(ops, lens, lens, 81)


def test_cross_attention_ragged(ops):
    ragged_case(ops, [1, 9, 70], [33, 300, 47], 82)
    ragged_case(ops, [1, 9, 60], [33, 300, 47], 83)        # below the switch: the fp32-MFMA kernel on the same key lengths


def large_range_inputs():
    """tests/test_gpu_ops.py::test_attention_large_score_range at d_k = 80: scores of magnitude ~500, every seventh key scaled by a
    factor growing from 0.2 to 3 with its position, so the running maximum keeps rising until the last tiles."""
    rng = np.random.default_rng(31)
    Q = (rng.standard_normal((300, H * DK)) * 6).astype(np.float32)
    K = (rng.standard_normal((400, H * DK)) * 6).astype(np.float32)
    K[np.arange(0, 400, 7)] *= np.linspace(0.2, 3.0, len(range(0, 400, 7)))[:, None].astype(np.float32)
    V = rng.standard_normal((400, H * DK)).astype(np.float32)
    return Q, K, V


@pytest.mark.parametrize("n_q", [300, 40])            # attention_h80.hip (lazy rescale) / attention_kernel<80, false> (rescale per tile)
def test_rescale_branch_and_large_score_range(ops, n_q):
    Q, K, V = large_range_inputs()
    Q = Q[:n_q]
    z = np.zeros(1, np.int32)
    O = ops.attention(dev(Q), dev(K), dev(V), dev(z), dev(np.asarray([n_q], np.int32)), dev(z), dev(np.asarray([400], np.int32)), H,
                      DK ** -0.5, head_dim=DK).cpu().numpy()
    ref = mha64(Q, K, V, H, DK)
    assert np.isfinite(O).all()
    err = float(np.abs(O - ref).max())
    print(f"d_k 80 large score range, {n_q} queries: max abs err {err:.3e}")
    assert err < 3e-4, err


def test_late_spike_forces_the_rescale(ops):
    """One late key dominates one query (the construction of test_gpu_ops.py's rescale case), in both kernels."""
    for q_lens, kv_lens, seed in (([140], [200], 84), ([40], [200], 85)):
        rng = np.random.default_rng(seed)
        Q = rng.standard_normal((q_lens[0], H * DK)).astype(np.float32)
        K = rng.standard_normal((kv_lens[0], H * DK)).astype(np.float32)
        V = rng.standard_normal((kv_lens[0], H * DK)).astype(np.float32)
        K[kv_lens[0] - 2, :DK] = Q[1, :DK] * 4
        z = np.zeros(1, np.int32)
        O = ops.attention(dev(Q), dev(K), dev(V), dev(z), dev(np.asarray(q_lens, np.int32)), dev(z), dev(np.asarray(kv_lens, np.int32)), H,
                          DK ** -0.5, head_dim=DK).cpu().numpy()
        err = float(np.abs(O - mha64(Q, K, V, H, DK)).max())
        print(f"d_k 80 late spike, {q_lens[0]} queries: max abs err {err:.3e}")
        assert err < 2e-5, err


def test_exact_form(ops):
    """The launch context set to exact (pfhip_op_set_launch_ctx), as the range guard's re-run sets it: every segment, the long ones
    included, runs the fp32-MFMA kernel — no fp16 plane is touched — and meets the same bounds."""
    with exact_ctx(ops):
        ragged_case(ops, SELF_LENS, SELF_LENS, 80)
        Q, K, V = large_range_inputs()
        z = np.zeros(1, np.int32)
        O = ops.attention(dev(Q), dev(K), dev(V), dev(z), dev(np.asarray([300], np.int32)), dev(z), dev(np.asarray([400], np.int32)), H,
                          DK ** -0.5, head_dim=DK).cpu().numpy()
    err = float(np.abs(O - mha64(Q, K, V, H, DK)).max())
    print(f"d_k 80 exact form, large score range: max abs err {err:.3e}")
    assert err < 3e-4, err


def test_exact_form_keeps_values_beyond_fp16_range(ops):
    """What makes the exact form exact: V of magnitude 1e6 overflows an fp16 plane (65504) but not the fp32 kernel."""
    rng = np.random.default_rng(86)
    Q = rng.standard_normal((100, H * DK)).astype(np.float32)
    K = rng.standard_normal((90, H * DK)).astype(np.float32)
    V = (rng.standard_normal((90, H * DK)) * 1e6).astype(np.float32)
    z = np.zeros(1, np.int32)
    with exact_ctx(ops):
        O = ops.attention(dev(Q), dev(K), dev(V), dev(z), dev(np.asarray([100], np.int32)), dev(z), dev(np.asarray([90], np.int32)), H,
                          DK ** -0.5, head_dim=DK).cpu().numpy()
    ref = mha64(Q, K, V, H, DK)
    assert np.isfinite(O).all() and np.abs(O - ref).max() < 2e-5 * 1e6


@pytest.mark.parametrize("Lq,Lk", [(20, 20), (1, 20), (20, 32), (7, 13)])
def test_window_attention(ops, Lq, Lk):
    """One streaming window at d_k = 80; Q / K / V as column blocks of one row-major buffer, as the streaming encoder hands them over."""
    rng = np.random.default_rng(Lq * 100 + Lk)
    d = H * DK
    qkv = (rng.standard_normal((32, 3 * d)) * 2.0).astype(np.float32)
    t = dev(qkv)
    out = ops.window_attention(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], Lq, Lk, H, DK ** -0.5, head_dim=DK).cpu().numpy()
    assert out.shape == (32, d)
    ref = mha64(qkv[:Lq, :d], qkv[:Lk, d:2 * d], qkv[:Lk, 2 * d:], H, DK)
    err = float(np.abs(out[:Lq] - ref).max())
    print(f"d_k 80 window attention {Lq} x {Lk}: max abs err {err:.3e}")
    assert err < 2e-5, err
    assert not out[Lq:].any()
    with pytest.raises(Exception):
        ops.window_attention(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], 33, 20, H, 1.0, head_dim=DK)


@pytest.mark.parametrize("head_dim", [64, 96])
def test_other_widths_are_refused_before_any_launch(ops, pkg, head_dim):
    d = H * head_dim
    sentinel = np.float32(-7.0)
    x = torch.full((32, 3 * d), 1.0, dtype=torch.float32, device="cuda")
    z = dev(np.zeros(1, np.int32))
    n = dev(np.asarray([32], np.int32))
    lib = pkg.load_lib()
    O = torch.full((32, d), float(sentinel), dtype=torch.float32, device="cuda")
    import ctypes
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    ops.window_attention(x[:, :H * 80], x[:, :H * 80], x[:, :H * 80], 1, 1, H, 1.0, head_dim=80)        # declares the argument types
    ops.attention(x[:, :H * 80], x[:, :H * 80], x[:, :H * 80], z, n, z, n, H, 1.0, head_dim=80)
    rc = lib.pfhip_op_attention_hd(p(x), 3 * d, p(x), 3 * d, p(x), 3 * d, p(O), d, p(z), p(n), p(z), p(n), 1, H, 32, ctypes.c_float(1.0), head_dim, None)
    assert rc != 0
    rc = lib.pfhip_op_window_attention_hd(p(x), 3 * d, p(x), 3 * d, p(x), 3 * d, p(O), d, 20, 20, H, ctypes.c_float(1.0), head_dim, None)
    assert rc != 0
    torch.cuda.synchronize()
    assert bool((O == float(sentinel)).all())                     # nothing was launched: the output is untouched
    with pytest.raises(pkg.PfhipError):
        ops.attention(x[:, :d], x[:, :d], x[:, :d], z, n, z, n, H, 1.0, head_dim=head_dim)
    with pytest.raises(pkg.PfhipError):
        ops.window_attention(x[:, :d], x[:, :d], x[:, :d], 20, 20, H, 1.0, head_dim=head_dim)
