"""GPU: the exact route of the d_k = 128 attention, selected the way the model selects it — through the launch context
(pfhip_op_set_launch_ctx(NULL, exact)) — and the lazy-rescale thresholds of every split-operand attention kernel, against
softmax(QK^T)V in fp64 per segment, through the operator-level C ABI (include/pfhip_ops.h).

  exact, more than 64 queries in the longest segment   attention_x6.hip: three bf16 planes, six products, its own copy of the fused SAN-M
                                                       memory block, lazy rescale when a maximum outgrows the reference by 2^16
  exact, up to 64 queries                              the fp32-MFMA attention_kernel<128, false> of attention.hip
  default context, more than 64 queries                attention_x3.hip / attention_p3.hip (d_k = 128), attention_h80.hip (d_k = 80):
                                                       two fp16 planes, lazy rescale at 2^10

The exact route is what the range guard re-runs a batch on when the fp16 two-plane kernels are out of their domain, so it is given what
it exists for: values beyond fp16's 65504 and rows far below 1.  Every operand is fp32 and the bf16 three-way split is exact for any
fp32 value, so scaling an operand by a power of two scales every product and every fp32 partial sum by it: the scaled runs must equal
the unscaled one bit for bit (nothing overflows or underflows at 2^+-18).

Tolerances are the project's figures for these forms (tests/test_gpu_ops.py): 2e-5 against fp64, 3e-4 for scores of magnitude ~500,
1e-5 for the memory block."""
import contextlib
import importlib

import numpy as np
import pytest

from attention_staircase import STAIR_K, STAIR_Q, staircase

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H, DK = 2, 128
D = H * DK
SELF_LENS = [1, 31, 32, 33, 64, 65, 257, 300]      # a single key, both sides of the 32-key tile, the 64-query switch, two 256-query workgroups
S = 18                                             # 2^18 N(0,1) reaches 1e6 (fp16: 65504); 2^-18 N(0,1) is 4e-6


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)


def i32(v):
    return dev(np.asarray(v, np.int32))


def mha64(q, k, v, n_head=H, dk=DK):
    q, k, v = (a.astype(np.float64) for a in (q, k, v))
    out = np.empty((q.shape[0], n_head * dk))
    for h in range(n_head):
        sl = slice(h * dk, (h + 1) * dk)
        s = q[:, sl] @ k[:, sl].T * dk ** -0.5
        p = np.exp(s - s.max(1, keepdims=True))
        out[:, sl] = (p / p.sum(1, keepdims=True)) @ v[:, sl]
    return out


def fsmn64(v, w):
    """The SAN-M memory block in fp64: v[t] + sum_j w[:, j] v[t + j - 5], zeros outside the segment."""
    v, w = v.astype(np.float64), w.astype(np.float64)
    T = v.shape[0]
    vp = np.zeros((T + 10, v.shape[1]))
    vp[5:5 + T] = v
    return v + sum(vp[j:j + T] * w[:, j][None, :] for j in range(11))


@contextlib.contextmanager
def exact_ctx(ops):
    ops.set_launch_ctx(None, True)
    try:
        yield
    finally:
        torch.cuda.synchronize()
        ops.set_launch_ctx()


def one_segment(ops, Q, K, V, n_head=H, dk=DK):
    z = np.zeros(1, np.int32)
    return ops.attention(dev(Q), dev(K), dev(V), dev(z), i32([Q.shape[0]]), dev(z), i32([K.shape[0]]), n_head, dk ** -0.5,
                         head_dim=dk).cpu().numpy()


# ---- ragged self- and cross-attention -----------------------------------------------------------------------------------------------
def ragged_case(ops, q_lens, kv_lens, seed, what):
    rng = np.random.default_rng(seed)
    q_off, kv_off = offsets(q_lens), offsets(kv_lens)
    Q = rng.standard_normal((sum(q_lens), D)).astype(np.float32)
    K = rng.standard_normal((sum(kv_lens), D)).astype(np.float32)
    V = rng.standard_normal((sum(kv_lens), D)).astype(np.float32)
    with exact_ctx(ops):
        O = ops.attention(dev(Q), dev(K), dev(V), dev(q_off), i32(q_lens), dev(kv_off), i32(kv_lens), H, DK ** -0.5).cpu().numpy()
    assert O.shape == (sum(q_lens), D) and np.isfinite(O).all()
    worst = 0.0
    for b in range(len(q_lens)):
        ref = mha64(Q[q_off[b]:q_off[b] + q_lens[b]], K[kv_off[b]:kv_off[b] + kv_lens[b]], V[kv_off[b]:kv_off[b] + kv_lens[b]])
        err = float(np.abs(O[q_off[b]:q_off[b] + q_lens[b]] - ref).max())
        print(f"exact {what}: segment {b} ({q_lens[b]} x {kv_lens[b]}) max abs err {err:.3e}")
        worst = max(worst, err)
    assert worst < 2e-5, worst


def test_exact_self_attention_ragged(ops):
    ragged_case(ops, SELF_LENS, SELF_LENS, 601, "self-attention (attention_x6.hip)")


def test_exact_self_attention_ragged_short_launch(ops):
    """No segment above 64 queries: under `exact` the whole launch is the fp32-MFMA kernel."""
    lens = [n for n in SELF_LENS if n <= 64]
    ragged_case(ops, lens, lens, 602, "self-attention (fp32-MFMA kernel)")


def test_exact_cross_attention_ragged(ops):
    ragged_case(ops, [3, 120, 1, 70], [17, 300, 64, 33], 603, "cross-attention (attention_x6.hip)")
    ragged_case(ops, [3, 60, 1, 64], [17, 300, 64, 33], 604, "cross-attention (fp32-MFMA kernel)")


# ---- the fused memory block under `exact` ---------------------------------------------------------------------------------------------
def test_exact_fused_memory_block(ops):
    """attention_x6.hip's own copy of the SAN-M memory block, reached through the launch context: the memory equals the stand-alone
    fsmn kernel's bit for bit (one rounding apart when added into the residual stream), the context equals the plain launch's bit for
    bit, rows behind the last utterance keep their sentinel."""
    rng = np.random.default_rng(605)
    lens, pad, sentinel = [1, 65, 257, 300], 64, -7.5
    off = offsets(lens)
    M = sum(lens)
    Q, K, V, X = (rng.standard_normal((M, D)).astype(np.float32) for _ in range(4))
    w = (rng.standard_normal((D, 11)) / 3).astype(np.float32)
    dl, doff = i32(lens), dev(off)
    assert ops.attention_fsmn_is_fused(max(lens), DK)
    with exact_ctx(ops):
        O = ops.attention(dev(Q), dev(K), dev(V), doff, dl, doff, dl, H, DK ** -0.5).cpu().numpy()
        runs = {}
        for acc in (False, True):
            mem0 = np.full((M + pad, D), sentinel, np.float32)
            mem0[:M] = X
            mem = dev(mem0)
            ctx = ops.attention_fsmn(dev(Q), dev(K), dev(V), doff, dl, H, DK ** -0.5, dev(w), mem, mem_accumulate=acc).cpu().numpy()
            runs[acc] = (ctx, mem.cpu().numpy())
    for b, (o, L) in enumerate(zip(off, lens)):
        err = float(np.abs(O[o:o + L] - mha64(Q[o:o + L], K[o:o + L], V[o:o + L])).max())
        assert err < 2e-5, (b, err)
    want_plain = ops.fsmn(dev(V), dev(w), doff, dl).cpu().numpy()
    for acc, (ctx, got_mem) in runs.items():
        worst = 0.0
        for o, L in zip(off, lens):
            ref = fsmn64(V[o:o + L], w) + (X[o:o + L].astype(np.float64) if acc else 0.0)
            worst = max(worst, float(np.abs(got_mem[o:o + L] - ref).max()))
        print(f"exact fused memory block, mem_accumulate {acc}: max abs err against fp64 {worst:.3e}")
        assert worst < 1e-5, (acc, worst)
        if not acc:
            assert np.array_equal(got_mem[:M], want_plain)
        assert np.array_equal(ctx, O)                    # the memory block does not disturb the attention
        assert np.all(got_mem[M:] == sentinel)


# ---- values the two-plane kernels cannot hold -------------------------------------------------------------------------------------------
def scaled_inputs(rows_q, rows_k, seed):
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((rows_q, D)).astype(np.float32)
    K = rng.standard_normal((rows_k, D)).astype(np.float32)
    V = rng.standard_normal((rows_k, D)).astype(np.float32)
    up, down = np.float32(2.0 ** S), np.float32(2.0 ** -S)
    # (name, Q, K, V, the power of two the result carries)
    return Q, K, V, [("V * 2^18", Q, K, V * up, 2.0 ** S), ("V * 2^-18", Q, K, V * down, 2.0 ** -S), ("Q * 2^-18, K * 2^18", Q * down, K * up, V, 1.0)]


@pytest.mark.parametrize("n_q", [100, 40])               # attention_x6.hip / the fp32-MFMA kernel
def test_exact_route_on_values_beyond_fp16(ops, n_q):
    """100 (40) queries x 90 keys.  Each scaled run equals the unscaled exact run times the same power of two BIT FOR BIT, and is
    within 2e-5 * 2^+-18 of fp64; in the default context V * 2^18 (up to 1e6 against fp16's 65504) is NOT served — which is what
    proves that the launch context routed the exact runs."""
    Q, K, V, variants = scaled_inputs(n_q, 90, 606)
    with exact_ctx(ops):
        base = one_segment(ops, Q, K, V)
        got = [one_segment(ops, q, k, v) for _, q, k, v, _ in variants]
    err = float(np.abs(base - mha64(Q, K, V)).max())
    print(f"exact, {n_q} x 90 unscaled: max abs err {err:.3e}")
    assert err < 2e-5, err
    for (name, q, k, v, f), o in zip(variants, got):
        assert np.isfinite(o).all(), name
        err = float(np.abs(o - mha64(q, k, v)).max())
        print(f"exact, {n_q} x 90, {name}: max abs err {err:.3e} = {err / f:.3e} x the scale; "
              f"{int((o != base * np.float32(f)).sum())} elements differ from the scaled unscaled run")
        assert err < 2e-5 * f, (name, err)
        assert np.array_equal(o, base * np.float32(f)), name
    if n_q > 64:      # the control: the same call outside the context runs the fp16 two-plane kernel, which cannot hold 2.6e5
        name, q, k, v, f = variants[0]
        o = one_segment(ops, q, k, v)
        served = bool(np.isfinite(o).all()) and float(np.abs(o - mha64(q, k, v)).max()) < 2e-5 * f
        assert not served, "the default context served V * 2^18: the launch context is not what routes the exact runs"


@pytest.mark.parametrize("L", [100, 40])                 # the fused launch on attention_x6.hip / fsmn + the fp32-MFMA kernel
def test_exact_route_on_values_beyond_fp16_with_memory_block(ops, L):
    """The same three variants through attention_fsmn (self-attention over L rows): context and memory scale bit for bit."""
    Q, K, V, variants = scaled_inputs(L, L, 607)
    w = (np.random.default_rng(608).standard_normal((D, 11)) / 3).astype(np.float32)
    z, dl = dev(np.zeros(1, np.int32)), i32([L])

    def run(q, k, v):
        mem = torch.zeros((L, D), dtype=torch.float32, device="cuda")
        ctx = ops.attention_fsmn(dev(q), dev(k), dev(v), z, dl, H, DK ** -0.5, dev(w), mem).cpu().numpy()
        return ctx, mem.cpu().numpy()

    with exact_ctx(ops):
        base_ctx, base_mem = run(Q, K, V)
        got = [run(q, k, v) for _, q, k, v, _ in variants]
    assert float(np.abs(base_ctx - mha64(Q, K, V)).max()) < 2e-5
    assert float(np.abs(base_mem - fsmn64(V, w)).max()) < 1e-5
    for (name, q, k, v, f), (ctx, mem) in zip(variants, got):
        err = float(np.abs(ctx - mha64(q, k, v)).max())
        merr = float(np.abs(mem - fsmn64(v, w)).max())
        print(f"exact attention_fsmn, {L} rows, {name}: context err {err:.3e}, memory err {merr:.3e}")
        assert err < 2e-5 * f and merr < 1e-5 * f, (name, err, merr)
        assert np.array_equal(ctx, base_ctx * np.float32(f)), name
        assert np.array_equal(mem, base_mem * np.float32(f)), name          # (the Q / K variant leaves V, hence the memory, alone)


# ---- large score range ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q", [300, 40])
def test_exact_large_score_range(ops, n_q):
    """The inputs of tests/test_gpu_ops.py::test_attention_large_score_range (scores of magnitude ~500, growing maxima) under `exact`."""
    rng = np.random.default_rng(31)
    Q = (rng.standard_normal((300, D)) * 6).astype(np.float32)[:n_q]
    K = (rng.standard_normal((400, D)) * 6).astype(np.float32)
    K[np.arange(0, 400, 7)] *= np.linspace(0.2, 3.0, len(range(0, 400, 7)))[:, None].astype(np.float32)
    V = rng.standard_normal((400, D)).astype(np.float32)
    with exact_ctx(ops):
        O = one_segment(ops, Q, K, V)
    assert np.isfinite(O).all()
    err = float(np.abs(O - mha64(Q, K, V)).max())
    print(f"exact large score range, {n_q} x 400: max abs err {err:.3e}")
    assert err < 3e-4, err


# ---- the lazy-rescale thresholds -----------------------------------------------------------------------------------------------------------
def kv_planes(ops, K, V):
    out = ops.split_rows(dev(K), ldp=2 * D)
    return ops.split_rows(dev(V), ldp=2 * D, out=out, col=D)


@pytest.mark.parametrize("step", [9.5, 10.5])
def test_staircase_default_context(ops, step):
    """m_run + 10 in attention_x3.hip (fp32 K / V) and attention_p3.hip (K | V as row-major fp16 planes)."""
    Q, K, V = staircase(step, DK, H)
    ref = mha64(Q, K, V)
    z, ql, kl = dev(np.zeros(1, np.int32)), i32([STAIR_Q]), i32([STAIR_K])
    got = one_segment(ops, Q, K, V)
    err = float(np.abs(got - ref).max())
    print(f"staircase step {step}, attention_x3.hip: max abs err {err:.3e} (query 1: {float(np.abs(got[1] - ref[1]).max()):.3e})")
    assert np.isfinite(got).all() and err < 2e-5, err
    got = ops.attention_kvplanes(dev(Q), kv_planes(ops, K, V), D, z, ql, z, kl, H, DK ** -0.5).cpu().numpy()
    err = float(np.abs(got - ref).max())
    print(f"staircase step {step}, attention_p3.hip: max abs err {err:.3e} (query 1: {float(np.abs(got[1] - ref[1]).max()):.3e})")
    assert np.isfinite(got).all() and err < 2e-5, err


@pytest.mark.parametrize("step", [15.5, 16.5])
def test_staircase_exact_context(ops, step):
    """m_run + 16 in attention_x6.hip: probabilities reach 2^15.5 = 4.6e4 before the reference moves."""
    Q, K, V = staircase(step, DK, H)
    with exact_ctx(ops):
        got = one_segment(ops, Q, K, V)
    ref = mha64(Q, K, V)
    err = float(np.abs(got - ref).max())
    print(f"staircase step {step}, attention_x6.hip: max abs err {err:.3e} (query 1: {float(np.abs(got[1] - ref[1]).max()):.3e})")
    assert np.isfinite(got).all() and err < 2e-5, err


@pytest.mark.parametrize("step", [9.5, 10.5])
def test_staircase_head_width_80(ops, step):
    """m_run + 10 in attention_h80.hip."""
    Q, K, V = staircase(step, 80, H)
    got = one_segment(ops, Q, K, V, H, 80)
    ref = mha64(Q, K, V, H, 80)
    err = float(np.abs(got - ref).max())
    print(f"staircase step {step}, attention_h80.hip: max abs err {err:.3e} (query 1: {float(np.abs(got[1] - ref[1]).max()):.3e})")
    assert np.isfinite(got).all() and err < 2e-5, err
