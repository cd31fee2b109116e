"""GPU: a round of streaming connections' windows in ONE launch — pfhip_op_window_attention_segments, i.e. stream_fused.hip's
window_attention_kernel with segment arrays, grid (H, B), and the SAN-M memory block of V written by the same launch (what the
streaming encoder and the decoder's cross-attention run for every round) — against softmax(QK^T)V and the FSMN in fp64 per window.

Q, K and V are column blocks of one [rows, 3 d] buffer as the streaming encoder hands them over (the decoder form: Q [rows, d], K | V
column blocks of a [rows, 2 d] buffer).  Rows of no window and rows behind the last window keep a sentinel.  The kernel body is the one
pfhip_op_window_attention launches for a single window, so each window's result must equal that launch's bit for bit; the memory
block claims launch_fsmn's operation order, so it must equal pfhip_op_fsmn's bit for bit.

Tolerances: 2e-5 (attention) and 1e-5 (memory block) against fp64, the project's figures for these forms (tests/test_gpu_ops.py)."""
import ctypes
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H = 4
SENTINEL = np.float32(-7.5)
SELF_LENS = [20, 1, 13, 32, 7, 2]
SELF_OFF = [0, 22, 23, 40, 72, 81]            # gaps of rows that belong to no window: 20-21, 36-39, 79-80; rows 83.. behind the last
SELF_ROWS = 96
WIDE = 3                                      # the window whose Q and K are scaled by 2: scores of several units


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def i32(v):
    return dev(np.asarray(v, np.int32))


def mha64(q, k, v, dk):
    q, k, v = (a.astype(np.float64) for a in (q, k, v))
    out = np.empty((q.shape[0], H * dk))
    for h in range(H):
        sl = slice(h * dk, (h + 1) * dk)
        s = q[:, sl] @ k[:, sl].T * dk ** -0.5
        p = np.exp(s - s.max(1, keepdims=True))
        out[:, sl] = (p / p.sum(1, keepdims=True)) @ v[:, sl]
    return out


def fsmn64(v, w):
    v, w = v.astype(np.float64), w.astype(np.float64)
    T = v.shape[0]
    vp = np.zeros((T + 10, v.shape[1]))
    vp[5:5 + T] = v
    return v + sum(vp[j:j + T] * w[:, j][None, :] for j in range(11))


def window_rows(offs, lens, rows):
    live = np.zeros(rows, bool)
    for o, n in zip(offs, lens):
        live[o:o + n] = True
    return live


def self_case(dk):
    rng = np.random.default_rng(700 + dk)
    d = H * dk
    qkv = rng.standard_normal((SELF_ROWS, 3 * d)).astype(np.float32)
    o, n = SELF_OFF[WIDE], SELF_LENS[WIDE]
    qkv[o:o + n, :2 * d] *= 2.0
    w = (rng.standard_normal((d, 11)) / 3).astype(np.float32)
    return d, qkv, w


@pytest.mark.parametrize("dk", [128, 80])
def test_self_attention_windows(ops, dk):
    d, qkv, _ = self_case(dk)
    t = dev(qkv)
    out = torch.full((SELF_ROWS, d), float(SENTINEL), dtype=torch.float32, device="cuda")
    ops.window_attention_segments(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], i32(SELF_OFF), i32(SELF_LENS), i32(SELF_OFF), i32(SELF_LENS), H,
                                  dk ** -0.5, head_dim=dk, out=out)
    got = out.cpu().numpy()
    for b, (o, n) in enumerate(zip(SELF_OFF, SELF_LENS)):
        ref = mha64(qkv[o:o + n, :d], qkv[o:o + n, d:2 * d], qkv[o:o + n, 2 * d:], dk)
        err = float(np.abs(got[o:o + n] - ref).max())
        print(f"d_k {dk} window segments, self-attention: window {b} ({n} x {n}) max abs err {err:.3e}")
        assert err < 2e-5, (b, err)
        alone = ops.window_attention(t[o:, :d], t[o:, d:2 * d], t[o:, 2 * d:], n, n, H, dk ** -0.5, head_dim=dk).cpu().numpy()
        assert np.array_equal(got[o:o + n], alone[:n]), b            # the same kernel body on the same rows
    assert np.all(got[~window_rows(SELF_OFF, SELF_LENS, SELF_ROWS)] == SENTINEL)


@pytest.mark.parametrize("dk", [128, 80])
def test_self_attention_windows_with_memory_block(ops, dk):
    """fsmn_w given: the launch also writes the SAN-M memory of V.  O and mem are allocated 8 columns wider than H * d_k: no column
    outside a head's own [h d_k, (h + 1) d_k) — none at or past H * d_k in particular — is written (at d_k = 80 half of wave 2's
    32-wide slice and all of wave 3's lie outside the head)."""
    d, qkv, w = self_case(dk)
    ld = d + 8
    t = dev(qkv)
    off, ln = i32(SELF_OFF), i32(SELF_LENS)
    plain = torch.full((SELF_ROWS, ld), float(SENTINEL), dtype=torch.float32, device="cuda")
    ops.window_attention_segments(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], off, ln, off, ln, H, dk ** -0.5, head_dim=dk, out=plain)
    out = torch.full((SELF_ROWS, ld), float(SENTINEL), dtype=torch.float32, device="cuda")
    mem = torch.full((SELF_ROWS, ld), float(SENTINEL), dtype=torch.float32, device="cuda")
    ops.window_attention_segments(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], off, ln, off, ln, H, dk ** -0.5, head_dim=dk, fsmn_w=dev(w), mem=mem,
                                  out=out)
    got, got_mem = out.cpu().numpy(), mem.cpu().numpy()
    assert np.array_equal(got, plain.cpu().numpy())                  # the context is unchanged by the presence of fsmn_w
    want = ops.fsmn(t[:, 2 * d:], dev(w), off, ln).cpu().numpy()
    live = window_rows(SELF_OFF, SELF_LENS, SELF_ROWS)
    assert np.array_equal(got_mem[live, :d], want[live])             # launch_fsmn's operation order
    worst = 0.0
    for o, n in zip(SELF_OFF, SELF_LENS):
        worst = max(worst, float(np.abs(got_mem[o:o + n, :d] - fsmn64(qkv[o:o + n, 2 * d:], w)).max()))
        assert float(np.abs(got[o:o + n, :d] - mha64(qkv[o:o + n, :d], qkv[o:o + n, d:2 * d], qkv[o:o + n, 2 * d:], dk)).max()) < 2e-5
    print(f"d_k {dk} window segments, memory block: max abs err against fp64 {worst:.3e}")
    assert worst < 1e-5, worst
    for a in (got, got_mem):
        assert np.all(a[~live] == SENTINEL) and np.all(a[:, d:] == SENTINEL)


@pytest.mark.parametrize("dk", [128, 80])
def test_cross_attention_windows(ops, dk):
    """The decoder form: a few tokens per connection against its window; a connection with no tokens writes nothing; odd key counts
    (13, 1) use half of the last MFMA step."""
    rng = np.random.default_rng(710 + dk)
    d = H * dk
    q_len, kv_len = [3, 0, 1, 20, 5], [20, 20, 13, 32, 1]
    q_off, kv_off = [0, 3, 5, 7, 28], [0, 20, 40, 53, 85]      # q rows 3-4 (where the empty window points), 6, 27 and 33.. belong to no window
    q_rows, kv_rows = 40, 90
    Q = rng.standard_normal((q_rows, d)).astype(np.float32)
    KV = rng.standard_normal((kv_rows, 2 * d)).astype(np.float32)
    tq, tkv = dev(Q), dev(KV)
    out = torch.full((q_rows, d), float(SENTINEL), dtype=torch.float32, device="cuda")
    ops.window_attention_segments(tq, tkv[:, :d], tkv[:, d:], i32(q_off), i32(q_len), i32(kv_off), i32(kv_len), H, dk ** -0.5, head_dim=dk,
                                  out=out)
    got = out.cpu().numpy()
    for b, (qo, qn, ko, kn) in enumerate(zip(q_off, q_len, kv_off, kv_len)):
        if qn == 0:
            continue
        ref = mha64(Q[qo:qo + qn], KV[ko:ko + kn, :d], KV[ko:ko + kn, d:], dk)
        err = float(np.abs(got[qo:qo + qn] - ref).max())
        print(f"d_k {dk} window segments, cross-attention: window {b} ({qn} x {kn}) max abs err {err:.3e}")
        assert err < 2e-5, (b, err)
        alone = ops.window_attention(tq[qo:], tkv[ko:, :d], tkv[ko:, d:], qn, kn, H, dk ** -0.5, head_dim=dk).cpu().numpy()
        assert np.array_equal(got[qo:qo + qn], alone[:qn]), b
    assert np.all(got[~window_rows(q_off, q_len, q_rows)] == SENTINEL)


def test_refuses_what_the_kernel_assumes(ops, pkg):
    """hipErrorInvalidValue (1) before anything is launched: the outputs keep their sentinel."""
    dk = 128
    d = H * dk
    t = torch.ones((32, 3 * d + 4), dtype=torch.float32, device="cuda")
    out = torch.full((32, d), float(SENTINEL), dtype=torch.float32, device="cuda")
    mem = torch.full((32, d), float(SENTINEL), dtype=torch.float32, device="cuda")
    w = torch.ones((d, 11), dtype=torch.float32, device="cuda")
    z, n = i32([0]), i32([20])
    ops.window_attention_segments(t[:, :d], t[:, d:2 * d], t[:, 2 * d:3 * d], z, n, z, n, H, 1.0, head_dim=dk)      # declares the argument types
    lib = pkg.load_lib()
    p = lambda a: ctypes.c_void_p(a.data_ptr()) if a is not None else None
    ld = t.stride(0)
    good = dict(Q=p(t), ldq=ld, K=p(t), ldk=ld, V=p(t), ldv=ld, O=p(out), ldo=d, q_off=p(z), q_len=p(n), kv_off=p(z), kv_len=p(n), B=1, H=H,
                max_q_len=20, max_kv_len=20, scale=ctypes.c_float(1.0), fsmn_w=None, mem=None, ldmem=0, head_dim=dk, stream=None)
    assert ld % 4 == 0
    bad = [dict(max_q_len=0), dict(max_q_len=33), dict(max_kv_len=0), dict(max_kv_len=33), dict(head_dim=64), dict(head_dim=32),
           dict(head_dim=96), dict(B=0), dict(H=0), dict(Q=None), dict(K=None), dict(V=None), dict(O=None), dict(q_off=None),
           dict(q_len=None), dict(kv_off=None), dict(kv_len=None), dict(ldq=ld + 2), dict(ldk=ld + 1), dict(ldv=ld + 2), dict(ldo=d + 2),
           dict(ldo=d - 4), dict(fsmn_w=p(w)), dict(fsmn_w=p(w), mem=p(mem), ldmem=d - 4), dict(fsmn_w=p(w), mem=p(mem), ldmem=d + 2)]
    for over in bad:
        rc = lib.pfhip_op_window_attention_segments(*{**good, **over}.values())
        assert rc == 1, (over, rc)
    torch.cuda.synchronize()
    assert bool((out == float(SENTINEL)).all()) and bool((mem == float(SENTINEL)).all())
    assert lib.pfhip_op_window_attention_segments(*{**good, "fsmn_w": p(w), "mem": p(mem), "ldmem": d}.values()) == 0      # and the good call runs
    torch.cuda.synchronize()
    assert bool((out[:20] != float(SENTINEL)).all()) and bool((mem[:20] != float(SENTINEL)).all()) and bool((out[20:] == float(SENTINEL)).all())
    with pytest.raises(pkg.PfhipError):
        ops.window_attention_segments(t[:, :d], t[:, d:2 * d], t[:, 2 * d:3 * d], z, i32([33]), z, n, H, 1.0, head_dim=dk)
