"""GPU: the two launches of every layer of the 256-wide online CT-Transformer (csrc/punc.cpp), each through its own operator entry
(include/pfhip_ops.h) against fp64:

  pfhip_op_attention_limit   the masked branch of attention.hip's fp32-MFMA kernel (q_kv_limit != NULL: EVERY tile takes the masked
                             path with a per-lane key limit), at head widths 32 (H = 8), 80 and 128 (H = 2)
  pfhip_op_fsmn_shift        fsmn_kernel<10>: the FSMN memory block with its taps shifted 5 frames into the past (fully causal)

Tolerances: 2e-5 (attention) and 1e-5 (memory block) against fp64, the project's figures for these kernels (tests/test_gpu_ops.py).
No limit of 0 is passed: CTTransformerOnline::VadMask never produces one, and the kernel's result for a row with no visible key is
undefined (include/pfhip_ops.h says so)."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

from oracle import ct_transformer as CT

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEG = [1, 33, 100, 140]                   # a single key, one key past a 32-key tile, several tiles, a segment across the 128-query block
OFF = np.concatenate([[0], np.cumsum(SEG)[:-1]]).astype(np.int32)
ROWS = int(sum(SEG))
SHAPES = [(8, 32), (2, 80), (2, 128)]
SENTINEL = np.float32(-7.5)


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def i32(v):
    return dev(np.asarray(v, np.int32))


@functools.lru_cache(maxsize=None)
def qkv_case(n_head, dk):
    rng = np.random.default_rng(800 + dk)
    d = n_head * dk
    return tuple(rng.standard_normal((ROWS, d)).astype(np.float32) for _ in range(3))


def masked64(q, k, v, n_head, dk, limit):
    """softmax(QK^T)V in fp64 where query i sees keys [0, limit[i]): -inf on the others."""
    q, k, v = (a.astype(np.float64) for a in (q, k, v))
    seen = np.arange(k.shape[0])[None, :] < np.asarray(limit)[:, None]
    out = np.empty((q.shape[0], n_head * dk))
    for h in range(n_head):
        sl = slice(h * dk, (h + 1) * dk)
        s = np.where(seen, q[:, sl] @ k[:, sl].T * dk ** -0.5, -np.inf)
        p = np.exp(s - s.max(1, keepdims=True))
        out[:, sl] = (p / p.sum(1, keepdims=True)) @ v[:, sl]
    return out


def vad_limits(L, vad_pos):
    """A VadMask as per-query key limits: every row of oracle.ct_transformer.vad_mask is a prefix of ones."""
    m = CT.vad_mask(L, vad_pos)
    lim = m.sum(1).astype(np.int32)
    assert np.array_equal(m > 0, np.arange(L)[None, :] < lim[:, None]) and lim.min() >= 1
    return lim


def run_limited(ops, n_head, dk, limits, what):
    """One packed launch over SEG with per-row limits (list per segment); the largest error against fp64 over all segments."""
    Q, K, V = qkv_case(n_head, dk)
    lim = np.concatenate(limits).astype(np.int32)
    ln = i32(SEG)
    got = ops.attention_limit(dev(Q), dev(K), dev(V), dev(OFF), ln, dev(OFF), ln, n_head, dk ** -0.5, dev(lim), head_dim=dk).cpu().numpy()
    assert np.isfinite(got).all()
    worst = 0.0
    for b, (o, L) in enumerate(zip(OFF, SEG)):
        ref = masked64(Q[o:o + L], K[o:o + L], V[o:o + L], n_head, dk, np.minimum(limits[b], L))
        err = float(np.abs(got[o:o + L] - ref).max())
        print(f"attention_limit H {n_head} d_k {dk}, {what}: segment {b} ({L} rows) max abs err {err:.3e}")
        worst = max(worst, err)
    return got, worst


@pytest.mark.parametrize("H,dk", SHAPES)
@pytest.mark.parametrize("where", ["start", "mid", "end"])
def test_vad_mask_limits(ops, H, dk, where):
    """VadMask rows at vad_pos 0 (no mask), mid-segment (rows before vad_pos - 1 see keys [0, vad_pos)) and L (no mask again)."""
    limits = [vad_limits(L, {"start": 0, "mid": L // 2, "end": L}[where]) for L in SEG]
    if where == "mid":
        assert any((lim < L).any() for lim, L in zip(limits, SEG))          # the mask masks
    else:
        assert all((lim == L).all() for lim, L in zip(limits, SEG))
    _, worst = run_limited(ops, H, dk, limits, f"vad_pos at {where}")
    assert worst < 2e-5, worst


@pytest.mark.parametrize("H,dk", SHAPES)
def test_random_limits(ops, H, dk):
    """Limits drawn from 1..L per row: neighbouring lanes of a wave differ, and limits fall inside and on the edges of the 32-key
    tiles (1, 32, 33, 64, 96 and L are planted), so whole tiles behind a row's limit are masked for that lane only."""
    rng = np.random.default_rng(810 + dk)
    limits = []
    for L in SEG:
        lim = rng.integers(1, L + 1, L)
        for i, edge in enumerate(e for e in (1, 32, 33, 64, 96, L, 31, 65) if e <= L):
            lim[(7 * i + 3) % L] = edge
        limits.append(lim.astype(np.int32))
    assert {1, 32, 33, 64, 96, 140} <= set(int(v) for v in limits[3])
    _, worst = run_limited(ops, H, dk, limits, "random limits")
    assert worst < 2e-5, worst


@pytest.mark.parametrize("H,dk", SHAPES)
def test_limit_at_or_past_the_segment_is_no_mask(ops, H, dk):
    """A limit >= L (L itself, and beyond it: the kernel clamps) gives the unmasked attention, within 2e-5 — not bit for bit: the
    masked path adds the two score accumulators before the maximum, and at d_k = 128 the plain launch is another kernel."""
    Q, K, V = qkv_case(H, dk)
    limits = [(L + 50 * (np.arange(L) % 3)).astype(np.int32) for L in SEG]
    got, worst = run_limited(ops, H, dk, limits, "limits >= L")
    assert worst < 2e-5, worst
    ln = i32(SEG)
    plain = ops.attention(dev(Q), dev(K), dev(V), dev(OFF), ln, dev(OFF), ln, H, dk ** -0.5, head_dim=dk).cpu().numpy()
    diff = float(np.abs(got - plain).max())
    print(f"attention_limit H {H} d_k {dk}, limits >= L against the unmasked launch: max abs diff {diff:.3e}")
    assert diff < 2e-5, diff


def test_attention_limit_refuses_what_the_kernel_assumes(ops, pkg):
    H, dk = 2, 128
    d = H * dk
    x = torch.ones((32, d + 4), dtype=torch.float32, device="cuda")
    out = torch.full((32, d), float(SENTINEL), dtype=torch.float32, device="cuda")
    z, n, lim = i32([0]), i32([32]), i32([32] * 32)
    ops.attention_limit(x[:, :d], x[:, :d], x[:, :d], z, n, z, n, H, 1.0, lim, head_dim=dk)          # declares the argument types
    lib = pkg.load_lib()
    p = lambda a: ctypes.c_void_p(a.data_ptr()) if a is not None else None
    ld = x.stride(0)
    good = dict(Q=p(x), ldq=ld, K=p(x), ldk=ld, V=p(x), ldv=ld, O=p(out), ldo=d, q_off=p(z), q_len=p(n), kv_off=p(z), kv_len=p(n), B=1, H=H,
                max_q_len=32, scale=ctypes.c_float(1.0), head_dim=dk, q_kv_limit=p(lim), stream=None)
    bad = [dict(head_dim=64), dict(head_dim=96), dict(head_dim=43), dict(H=0), dict(Q=None), dict(K=None), dict(V=None), dict(O=None),
           dict(q_off=None), dict(q_len=None), dict(kv_off=None), dict(kv_len=None), dict(q_kv_limit=None), dict(ldq=ld + 2), dict(ldk=ld + 1),
           dict(ldv=ld + 3), dict(ldo=d + 2), dict(ldo=d - 4)]
    for over in bad:
        rc = lib.pfhip_op_attention_limit(*{**good, **over}.values())
        assert rc == 1, (over, rc)
    torch.cuda.synchronize()
    assert bool((out == float(SENTINEL)).all())                      # nothing was launched
    assert lib.pfhip_op_attention_limit(*good.values()) == 0
    torch.cuda.synchronize()
    assert bool((out != float(SENTINEL)).all())
    with pytest.raises(pkg.PfhipError):
        ops.attention_limit(x[:, :256], x[:, :256], x[:, :256], z, n, z, n, 4, 1.0, lim, head_dim=64)


# ---- the shifted FSMN -------------------------------------------------------------------------------------------------------------------
FSMN_LENS = [1, 5, 6, 10, 11, 16, 17, 40]      # both sides of the 10-frame look-back and of the 16-frame time tile
FSMN_OFF = np.concatenate([[0], np.cumsum(FSMN_LENS)[:-1]]).astype(np.int32)
FSMN_ROWS = int(sum(FSMN_LENS))


def fsmn_shift64(v, w, shift):
    """v[t] + sum_j w[:, j] v[t + j - 5 - shift] in fp64, zeros outside the segment: taps over [t - 10, t] at shift 5."""
    v, w = v.astype(np.float64), w.astype(np.float64)
    T = v.shape[0]
    vp = np.zeros((T + 10, v.shape[1]))
    vp[5 + shift:5 + shift + T] = v
    return v + sum(vp[j:j + T] * w[:, j][None, :] for j in range(11))


@functools.lru_cache(maxsize=None)
def fsmn_case(C):
    rng = np.random.default_rng(820 + C)
    v = rng.standard_normal((FSMN_ROWS, C)).astype(np.float32)
    res = rng.standard_normal((FSMN_ROWS, C)).astype(np.float32)
    w = (rng.standard_normal((C, 11)) / 3).astype(np.float32)
    return v, res, w


@pytest.mark.parametrize("C", [256, 516])
@pytest.mark.parametrize("use_res", [False, True])
def test_fsmn_shift_causal(ops, C, use_res):
    v, res, w = fsmn_case(C)
    off, ln = dev(FSMN_OFF), i32(FSMN_LENS)
    got = ops.fsmn_shift(dev(v), dev(w), off, ln, 5, res=dev(res) if use_res else None).cpu().numpy()
    worst = worst_oracle = 0.0
    for o, L in zip(FSMN_OFF, FSMN_LENS):
        extra = res[o:o + L].astype(np.float64) if use_res else 0.0
        worst = max(worst, float(np.abs(got[o:o + L] - (fsmn_shift64(v[o:o + L], w, 5) + extra)).max()))
        # the oracle's shifted block (fp32, another summation order): the same bound
        worst_oracle = max(worst_oracle, float(np.abs(got[o:o + L] - (CT.fsmn_shift(v[o:o + L], w, 5).astype(np.float64) + extra)).max()))
    print(f"fsmn_shift C {C} shift 5 residual {use_res}: max abs err against fp64 {worst:.3e}, against the oracle {worst_oracle:.3e}")
    assert worst < 1e-5 and worst_oracle < 1e-5, (worst, worst_oracle)
    assert float(np.abs(fsmn_shift64(v[-40:], w, 5) - fsmn_shift64(v[-40:], w, 0)).max()) > 0.1          # the shift matters


@pytest.mark.parametrize("C", [256, 516])
@pytest.mark.parametrize("use_res", [False, True])
def test_fsmn_shift_zero_is_fsmn(ops, C, use_res):
    v, res, w = fsmn_case(C)
    off, ln = dev(FSMN_OFF), i32(FSMN_LENS)
    r = dev(res) if use_res else None
    got = ops.fsmn_shift(dev(v), dev(w), off, ln, 0, res=r).cpu().numpy()
    assert np.array_equal(got, ops.fsmn(dev(v), dev(w), off, ln, res=r).cpu().numpy())
    o, L = int(FSMN_OFF[-1]), FSMN_LENS[-1]
    assert float(np.abs(got[o:o + L] - (fsmn_shift64(v[o:o + L], w, 0) + (res[o:o + L] if use_res else 0.0))).max()) < 1e-5


@pytest.mark.parametrize("C", [256, 516])
def test_fsmn_shift_is_causal_bit_for_bit(ops, C):
    """shift 5: out[t] does not depend on v[t + 1:].  t = 15 is the last frame of a 16-frame tile (the frames behind it are in the
    registers of the same thread), t = 20 sits inside the second tile."""
    v, _, w = fsmn_case(C)
    off, ln = dev(FSMN_OFF), i32(FSMN_LENS)
    base = ops.fsmn_shift(dev(v), dev(w), off, ln, 5).cpu().numpy()
    o, L = int(FSMN_OFF[-1]), FSMN_LENS[-1]
    for t in (15, 20):
        v2 = v.copy()
        v2[o + t + 1:o + L] = 1e3 * (1 + np.arange(L - t - 1, dtype=np.float32))[:, None]
        got = ops.fsmn_shift(dev(v2), dev(w), off, ln, 5).cpu().numpy()
        assert np.array_equal(got[:o + t + 1], base[:o + t + 1]), t
        assert not np.array_equal(got[o + t + 1], base[o + t + 1])


def test_fsmn_shift_refuses_what_the_kernel_assumes(ops, pkg):
    C = 256
    x = torch.ones((16, C + 4), dtype=torch.float32, device="cuda")
    w = torch.ones((C + 4, 11), dtype=torch.float32, device="cuda")
    out = torch.full((16, C + 4), float(SENTINEL), dtype=torch.float32, device="cuda")
    z, n = i32([0]), i32([16])
    ops.fsmn_shift(x[:, :C], w, z, n, 5)                                         # declares the argument types
    lib = pkg.load_lib()
    p = lambda a: ctypes.c_void_p(a.data_ptr()) if a is not None else None
    ld = x.stride(0)
    good = dict(v=p(x), ldv=ld, w=p(w), res=None, ldres=0, out=p(out), ldo=ld, off=p(z), len=p(n), B=1, max_len=16, C=C, shift=5, stream=None)
    bad = [dict(shift=1), dict(shift=-5), dict(shift=10), dict(C=C + 2), dict(C=0), dict(v=None), dict(w=None), dict(out=None), dict(off=None),
           dict(len=None), dict(ldv=ld + 2), dict(ldo=ld + 1), dict(ldv=C - 4), dict(res=p(x), ldres=ld + 2)]
    for over in bad:
        rc = lib.pfhip_op_fsmn_shift(*{**good, **over}.values())
        assert rc == 1, (over, rc)
    torch.cuda.synchronize()
    assert bool((out == float(SENTINEL)).all())                      # nothing was launched
    assert lib.pfhip_op_fsmn_shift(*good.values()) == 0
    torch.cuda.synchronize()
    assert bool((out[:, :C] != float(SENTINEL)).all()) and bool((out[:, C:] == float(SENTINEL)).all())
    with pytest.raises(pkg.PfhipError):
        ops.fsmn_shift(x[:, :C], w, z, n, 3)
