"""GPU: pfhip_op_attention_dk (the exact-width form of attention.hip's kernel) — fp32 fused attention for head widths that are
not 32, 80 or 128 — against the fp64 product of oracle.paraformer.mha, as tests/test_gpu_punc.py::test_attention_head_dim_32_op holds the d_k = 32 form.

Q, K and V are column slices of one standard-normal [rows, 3 H d_k] matrix, so head h starts at column h * d_k of a row of
3 H d_k floats: as unaligned as in the model (d_k = 43: 4 bytes).  One packed call holds segments of 1, 31, 32, 33, 100 and 129
rows: a lone key, both sides of the 32-key tile edge and the second 128-query block.  Tolerance 2e-5 absolute, the project's bar
for its fp32 attention operators (test_gpu_punc.py, test_gpu_attention_hd80.py).  The output has a row stride of H d_k + 8, more
rows than are used and a sentinel everywhere: every pad column and unused row must still hold it."""
import ctypes
import importlib

import numpy as np
import pytest

from oracle import ct_transformer as C

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SHAPES = [(12, 43), (4, 24), (3, 40), (3, 64)]
LENS = [1, 31, 32, 33, 100, 129]
OFF = np.concatenate([[0], np.cumsum(LENS)[:-1]]).astype(np.int32)
ROWS = int(sum(LENS))
EXTRA_ROWS = 5
SENTINEL = -7.0
TOL = 2e-5
VAD_POS = 37                 # the cut of the 100-row segment


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_cases = {}


def case(H, dk):
    """Inputs and the fp64 references of one shape, computed once and shared by the tests of that shape."""
    if (H, dk) not in _cases:
        d = H * dk
        qkv = np.random.default_rng(1000 * H + dk).standard_normal((ROWS, 3 * d)).astype(np.float32)
        q64, k64, v64 = (qkv[:, i * d:(i + 1) * d].astype(np.float64) for i in range(3))
        ref = np.zeros((ROWS, d), np.float64)
        for o, L in zip(OFF, LENS):
            ref[o:o + L] = mha64(q64[o:o + L], k64[o:o + L], v64[o:o + L], H, None)
        o, L = int(OFF[4]), LENS[4]
        ref_masked = mha64(q64[o:o + L], k64[o:o + L], v64[o:o + L], H, C.vad_mask(L, VAD_POS))
        _cases[(H, dk)] = (qkv, ref, ref_masked)
    return _cases[(H, dk)]


def mha64(q, k, v, H, mask):
    """oracle.paraformer.mha's product in fp64 throughout; with a mask, oracle.ct_transformer.vad_mask's zeros are -inf scores."""
    dk = q.shape[1] // H
    out = np.empty(q.shape, np.float64)
    for h in range(H):
        sl = slice(h * dk, (h + 1) * dk)
        s = (q[:, sl] * dk ** -0.5) @ k[:, sl].T
        if mask is not None:
            s = np.where(mask > 0, s, -np.inf)
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        out[:, sl] = (e / e.sum(axis=-1, keepdims=True)) @ v[:, sl]
    return out


def sentinel_out(H, dk):
    return torch.full((ROWS + EXTRA_ROWS, H * dk + 8), SENTINEL, dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("H,dk", SHAPES)
def test_packed_segments_against_fp64(ops, H, dk):
    qkv, ref, _ = case(H, dk)
    d = H * dk
    t = dev(qkv)
    off, ln = dev(OFF), dev(np.asarray(LENS, np.int32))
    O = sentinel_out(H, dk)
    ops.attention_dk(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], off, ln, off, ln, H, dk ** -0.5, dk, out=O)
    got = O.cpu().numpy()
    for o, L in zip(OFF, LENS):
        err = float(np.abs(got[o:o + L, :d] - ref[o:o + L]).max())
        print(f"attention_dk H {H} d_k {dk} segment of {L}: max abs err {err:.3e}")
        assert err < TOL, (H, dk, L, err)
    # nothing else is written: the 8 pad columns of every row and the rows past the last segment
    assert (got[:, d:] == SENTINEL).all() and (got[ROWS:] == SENTINEL).all()


@pytest.mark.parametrize("H,dk", SHAPES)
def test_per_query_key_limit(ops, H, dk):
    """The 100-row segment with the limits punc_infer_packed builds for vad_pos = 37: rows before vad_pos - 1 see keys [0, vad_pos),
    all other rows see everything."""
    qkv, ref, ref_masked = case(H, dk)
    d = H * dk
    o, L = int(OFF[4]), LENS[4]
    t = dev(qkv)
    lim = np.full(ROWS, -1, np.int32)              # indexed by packed row; only the segment's rows are read
    lim[o:o + L] = [VAD_POS if i < VAD_POS - 1 else L for i in range(L)]
    off, ln = dev(np.asarray([o], np.int32)), dev(np.asarray([L], np.int32))
    O = sentinel_out(H, dk)
    ops.attention_dk(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], off, ln, off, ln, H, dk ** -0.5, dk, q_kv_limit=dev(lim), out=O)
    got = O.cpu().numpy()
    err = float(np.abs(got[o:o + L, :d] - ref_masked).max())
    print(f"attention_dk H {H} d_k {dk} with key limits: max abs err {err:.3e}")
    assert err < TOL, (H, dk, err)
    assert np.abs(ref_masked[:VAD_POS - 1] - ref[o:o + VAD_POS - 1]).max() > 1e-3          # the mask matters
    assert (got[:o] == SENTINEL).all() and (got[o + L:] == SENTINEL).all() and (got[:, d:] == SENTINEL).all()


def test_exact_width_form_equals_aligned_form_at_32(ops):
    """d_k = 32 is served by both forms of the kernel: the same products in the same order, so the same bits.  The slices of a
    [rows, 3 * 8 * 32] matrix are 16-byte aligned with a stride that is a multiple of 4, which the aligned form asks for."""
    H, dk = 8, 32
    qkv, _, _ = case(H, dk)
    d = H * dk
    t = dev(qkv)
    off, ln = dev(OFF), dev(np.asarray(LENS, np.int32))
    q, k, v = t[:, :d], t[:, d:2 * d], t[:, 2 * d:]
    exact = ops.attention_dk(q, k, v, off, ln, off, ln, H, dk ** -0.5, dk)
    aligned = ops.attention(q, k, v, off, ln, off, ln, H, dk ** -0.5, head_dim=dk)
    print(f"exact-width against aligned form, d_k 32: max abs diff {float((exact - aligned).abs().max()):.3e}")
    assert exact.shape == aligned.shape == (ROWS, d) and torch.equal(exact, aligned)


def test_exact_width_form_equals_aligned_form_at_32_with_key_limits(ops):
    """The same on the 100-row segment under the vad_pos = 37 limits of test_per_query_key_limit."""
    H, dk = 8, 32
    qkv, _, _ = case(H, dk)
    d = H * dk
    o, L = int(OFF[4]), LENS[4]
    t = dev(qkv)
    lim = np.full(ROWS, -1, np.int32)
    lim[o:o + L] = [VAD_POS if i < VAD_POS - 1 else L for i in range(L)]
    lim = dev(lim)
    off, ln = dev(np.asarray([o], np.int32)), dev(np.asarray([L], np.int32))
    q, k, v = t[:, :d], t[:, d:2 * d], t[:, 2 * d:]
    exact = ops.attention_dk(q, k, v, off, ln, off, ln, H, dk ** -0.5, dk, q_kv_limit=lim)
    aligned = ops.attention_limit(q, k, v, off, ln, off, ln, H, dk ** -0.5, lim, head_dim=dk)
    print(f"exact-width against aligned form, d_k 32, key limits: max abs diff {float((exact - aligned).abs().max()):.3e}")
    assert torch.equal(exact[o:o + L], aligned[o:o + L])
    assert bool((exact[o:o + L] != 0).any())          # (both start from zeros: the segment was written)


def test_empty_key_segment_writes_nothing(ops):
    """kv_len = 0 in the exact-width form: the kernel returns before any load, and no element of the output is written."""
    H, dk = 12, 43
    qkv, _, _ = case(H, dk)
    d = H * dk
    t = dev(qkv)
    off, q_len, kv_len = dev(np.asarray([0], np.int32)), dev(np.asarray([33], np.int32)), dev(np.asarray([0], np.int32))
    O = sentinel_out(H, dk)
    ops.attention_dk(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], off, q_len, off, kv_len, H, dk ** -0.5, dk, out=O)
    torch.cuda.synchronize()
    assert bool((O == SENTINEL).all())


def test_refusals_launch_nothing(ops, pkg):
    H, dk = 12, 43
    qkv, _, _ = case(H, dk)
    d = H * dk
    t = dev(qkv)
    off, ln = dev(OFF), dev(np.asarray(LENS, np.int32))
    O = sentinel_out(H, dk)
    ops.attention_dk(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], off, ln, off, ln, H, dk ** -0.5, dk)      # a good call first: what follows is refused, not broken
    lib = pkg.load_lib()
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    q, k, v = t[:, :d], t[:, d:2 * d], t[:, 2 * d:]

    def call(d_k, ldq):
        return lib.pfhip_op_attention_dk(p(q), ldq, p(k), 3 * d, p(v), 3 * d, p(O), O.stride(0), p(off), p(ln), p(off), p(ln), len(LENS), H,
                                         max(LENS), ctypes.c_float(1.0), d_k, None, None)

    assert call(0, 3 * d) != 0
    assert call(65, 3 * d) != 0
    assert call(dk, d - 1) != 0
    # the operator for the widths attention.hip is built for still refuses 43
    assert lib.pfhip_op_attention_hd(p(q), 3 * d, p(k), 3 * d, p(v), 3 * d, p(O), O.stride(0), p(off), p(ln), p(off), p(ln), len(LENS), H,
                                     max(LENS), ctypes.c_float(1.0), dk, None) != 0
    with pytest.raises(pkg.PfhipError):
        ops.attention_dk(q, k, v, off, ln, off, ln, H, 1.0, 65, out=O)
    with pytest.raises(pkg.PfhipError):
        ops.attention(q, k, v, off, ln, off, ln, H, 1.0, head_dim=dk)
    torch.cuda.synchronize()
    assert bool((O == SENTINEL).all())
