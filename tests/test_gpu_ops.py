"""GPU: each hand-written kernel against the oracle (numpy fp32) through the operator-level C ABI
(include/pfhip_ops.h).  Tolerances are stated per test; integer outputs must be exact."""
import importlib

import numpy as np
import pytest

from oracle import paraformer as P

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pad_rows(a, m=128):
    r = (a.shape[0] + m - 1) // m * m
    out = np.zeros((r,) + a.shape[1:], a.dtype)
    out[:a.shape[0]] = a
    return out


# fp32 MFMA == fmaf chain; only the summation order differs from OpenBLAS: |err| <~ 1e-6 * sqrt(K) * |terms|
@pytest.mark.parametrize("M,N,K", [(1, 128, 32), (128, 128, 32), (130, 512, 512), (500, 1536, 576),
                                   (257, 1003, 512), (16, 512, 2048), (1000, 2048, 512)])
@pytest.mark.parametrize("guard", [True, False])
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, 5, 8, 9, 10])    # by size / 128x128 / weight-streaming / 64x128 / bf16 split 256x128, 128x128 / fp16 split 256x128, 128x128, 64x128
def test_gemm_matches_numpy(ops, M, N, K, guard, kind):
    rng = np.random.default_rng(M * 7 + N)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    R1 = rng.standard_normal((M, N)).astype(np.float32)
    R2 = rng.standard_normal((M, N)).astype(np.float32)
    Np = (N + 127) // 128 * 128
    dA, dW = dev(pad_rows(A)), dev(pad_rows(W))
    dbias = dev(np.concatenate([bias, np.zeros(Np - N, np.float32)]))
    dR1 = dev(np.pad(pad_rows(R1), ((0, 0), (0, Np - N))))
    dR2 = dev(np.pad(pad_rows(R2), ((0, 0), (0, Np - N))))
    for (b, r1, r2, relu) in [(None, None, None, False), (dbias, None, None, True), (dbias, dR1, None, False),
                              (dbias, dR1, dR2, False), (None, dR1, None, True)]:
        if kind in (1, 3) and not guard and (N % 128):
            continue                                   # the unguarded tiled kernels are for padded shapes only
        C = ops.gemm_f32(dA, dW, bias=b, R1=r1, R2=r2, relu=relu, M=M, N=N, guard=guard, kind=kind).cpu().numpy()[:M, :N]
        ref = A @ W.T
        if b is not None:
            ref = ref + bias
        if r1 is not None:
            ref = ref + R1
        if r2 is not None:
            ref = ref + R2
        if relu:
            ref = np.maximum(ref, 0)
        assert np.abs(C - ref).max() < 2e-5 * max(1.0, np.sqrt(K / 512)), (M, N, K, kind)


def test_gemm_exact_integer_layout(ops):
    """A = I-like with ASYMMETRIC integer W: catches any row/col swap of the MFMA C/D map bit-exactly."""
    M, N, K = 256, 256, 64
    A = np.zeros((M, K), np.float32)
    for i in range(M):
        A[i, i % K] = 1 + (i // K)
    W = (np.arange(N)[:, None] * 3 + np.arange(K)[None, :] * 5 + 1).astype(np.float32)
    C = ops.gemm_f32(dev(A), dev(W)).cpu().numpy()
    assert np.array_equal(C, A @ W.T)


def test_gemm_in_place_residual(ops):
    rng = np.random.default_rng(3)
    A = rng.standard_normal((256, 512)).astype(np.float32)
    W = (rng.standard_normal((512, 512)) / 22).astype(np.float32)
    X = rng.standard_normal((256, 512)).astype(np.float32)
    dX = dev(X)
    ops.gemm_f32(dev(A), dev(W), R1=dX, out=dX, guard=False)
    assert np.abs(dX.cpu().numpy() - (A @ W.T + X)).max() < 2e-5


@pytest.mark.parametrize("D,Dout", [(512, 512), (560, 576), (2048, 2048)])
def test_layernorm(ops, D, Dout):
    rng = np.random.default_rng(D)
    x = (rng.standard_normal((37, D)) * 3 + 1).astype(np.float32)
    g = rng.standard_normal(D).astype(np.float32)
    b = rng.standard_normal(D).astype(np.float32)
    xin = np.zeros((37, Dout), np.float32)
    xin[:, :D] = x
    y = ops.layernorm(dev(xin), dev(g), dev(b), D=D, Dout=Dout).cpu().numpy()
    assert np.abs(y[:, :D] - P.layer_norm(x, g, b)).max() < 1e-5
    assert np.all(y[:, D:] == 0)


def test_fsmn_ragged_segments(ops):
    rng = np.random.default_rng(5)
    lens = [1, 7, 16, 17, 40, 3]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    M = sum(lens)
    v = rng.standard_normal((M, 512)).astype(np.float32)
    res = rng.standard_normal((M, 512)).astype(np.float32)
    w = (rng.standard_normal((512, 11)) / 3).astype(np.float32)
    for use_res in (False, True):
        out = ops.fsmn(dev(v), dev(w), dev(off), dev(np.asarray(lens, np.int32)), res=dev(res) if use_res else None).cpu().numpy()
        for o, L in zip(off, lens):
            ref = P.fsmn(v[o:o + L], w) + (res[o:o + L] if use_res else 0)
            assert np.abs(out[o:o + L] - ref).max() < 1e-5


def _attn_case(ops, q_lens, kv_lens, seed, spike=False):
    rng = np.random.default_rng(seed)
    H, dk = 4, 128
    q_off = np.concatenate([[0], np.cumsum(q_lens)[:-1]]).astype(np.int32)
    kv_off = np.concatenate([[0], np.cumsum(kv_lens)[:-1]]).astype(np.int32)
    Q = rng.standard_normal((sum(q_lens), H * dk)).astype(np.float32)
    K = rng.standard_normal((sum(kv_lens), H * dk)).astype(np.float32)
    V = rng.standard_normal((sum(kv_lens), H * dk)).astype(np.float32)
    if spike:     # force the online-softmax rescale branch: one late key dominates one query
        K[kv_off[0] + kv_lens[0] - 2, :dk] = Q[q_off[0] + 1, :dk] * 4
    O = ops.attention(dev(Q), dev(K), dev(V), dev(q_off), dev(np.asarray(q_lens, np.int32)), dev(kv_off),
                      dev(np.asarray(kv_lens, np.int32)), H, dk ** -0.5).cpu().numpy()
    for b in range(len(q_lens)):
        q = Q[q_off[b]:q_off[b] + q_lens[b]]
        k = K[kv_off[b]:kv_off[b] + kv_lens[b]]
        vv = V[kv_off[b]:kv_off[b] + kv_lens[b]]
        ref = P.mha(q.astype(np.float64), k.astype(np.float64), vv.astype(np.float64), H)
        got = O[q_off[b]:q_off[b] + q_lens[b]]
        assert np.abs(got - ref).max() < 2e-5, (b, np.abs(got - ref).max())


def test_attention_self_ragged(ops):
    lens = [1, 31, 32, 33, 100, 129, 500]
    _attn_case(ops, lens, lens, 11)


def test_attention_cross_ragged(ops):
    _attn_case(ops, [3, 120, 1, 40], [17, 500, 64, 33], 12)


def test_attention_rescale_branch(ops):
    _attn_case(ops, [40], [200], 13, spike=True)


def test_attention_self_with_fused_memory_block(ops):
    """The encoder layer's fused launch (attention_x3.hip; attention_x6.hip under PFHIP_ATT_X3=0; fsmn + attention under PFHIP_ATT_X6=0):
    the SAN-M memory of V equals the stand-alone fsmn kernel's bit for bit (same operation order; one rounding apart when it is added
    into the residual stream), the context equals the plain attention launch's bit for bit, rows behind the last utterance are untouched.
    Lengths: 1 (inside a launch whose longest segment exceeds 64), 65 (the shortest fused launch), 257 (past the 256-query workgroup and
    a 16-row strip), 300 (partial last key tile, strips that end mid-strip)."""
    rng = np.random.default_rng(41)
    H, dk, pad, sentinel = 2, 128, 128, -7.5
    D = H * dk
    lens = [1, 65, 257, 300]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    M = sum(lens)
    Q = rng.standard_normal((M, D)).astype(np.float32)
    K = rng.standard_normal((M, D)).astype(np.float32)
    V = rng.standard_normal((M, D)).astype(np.float32)
    X = rng.standard_normal((M, D)).astype(np.float32)
    w = (rng.standard_normal((D, 11)) / 3).astype(np.float32)
    dl, doff = dev(np.asarray(lens, np.int32)), dev(off)
    O = ops.attention(dev(Q), dev(K), dev(V), doff, dl, doff, dl, H, dk ** -0.5).cpu().numpy()
    for b, (o, L) in enumerate(zip(off, lens)):
        ref = P.mha(Q[o:o + L].astype(np.float64), K[o:o + L].astype(np.float64), V[o:o + L].astype(np.float64), H)
        assert np.abs(O[o:o + L] - ref).max() < 2e-5, (b, np.abs(O[o:o + L] - ref).max())
    fused = ops.attention_fsmn_is_fused(max(lens), dk)
    for acc in (False, True):
        if acc and not fused:      # the unfused pair ignores the flag
            continue
        mem0 = np.full((M + pad, D), sentinel, np.float32)
        mem0[:M] = X
        mem = dev(mem0)
        ctx = ops.attention_fsmn(dev(Q), dev(K), dev(V), doff, dl, H, dk ** -0.5, dev(w), mem, mem_accumulate=acc).cpu().numpy()
        got_mem = mem.cpu().numpy()
        want = ops.fsmn(dev(V), dev(w), doff, dl, res=dev(X) if acc else None).cpu().numpy()
        if acc:      # x + (v + conv) against (v + conv) + x: one rounding apart
            assert np.abs(got_mem[:M] - want).max() < 1e-5
        else:
            assert np.array_equal(got_mem[:M], want)
        for o, L in zip(off, lens):
            ref = P.fsmn(V[o:o + L].astype(np.float64), w.astype(np.float64)) + (X[o:o + L] if acc else 0)
            assert np.abs(got_mem[o:o + L] - ref).max() < 1e-5
        assert np.array_equal(ctx, O)      # the memory block does not disturb the attention
        assert np.all(got_mem[M:] == sentinel)


def test_attention_context_as_plane_images(ops):
    """attention_x3.hip writing the context as the fp16 plane images gemm_p3.hip stages by DMA: the decoded planes equal the fp32
    output of the same launch to the planes' 22 bits, rows of other utterances and pad rows untouched, and the images feed the
    output projection (gemm_p3) directly."""
    rng = np.random.default_rng(31)
    H, dk = 4, 128
    lens = [70, 300, 129, 500, 65]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    M = sum(lens)
    Q = rng.standard_normal((M, H * dk)).astype(np.float32)
    K = rng.standard_normal((M, H * dk)).astype(np.float32)
    V = rng.standard_normal((M, H * dk)).astype(np.float32)
    dl = dev(np.asarray(lens, np.int32))
    O = ops.attention(dev(Q), dev(K), dev(V), dev(off), dl, dev(off), dl, H, dk ** -0.5).cpu().numpy()
    hi, lo, rows = ops.attention_planes(dev(Q), dev(K), dev(V), dev(off), dl, dev(off), dl, H, dk ** -0.5)
    got = ops.planes_to_float(hi, lo, rows, H * dk)
    assert rows == (M + 127) // 128 * 128
    assert np.abs(got[:M] - O).max() <= 2.0 ** -22 * np.abs(O).max() + 2.0 ** -24
    assert np.abs(got[M:]).max() == 0                      # pad rows of the (zero-filled) image were not written
    W = (rng.standard_normal((512, 512)) / np.sqrt(512)).astype(np.float32)
    ws = ops.best_w_scale(float(np.abs(W).max()))
    C, _ = ops.gemm_p3((hi, lo, rows), ops.split_planes(dev(W), scale=ws), M, 512, 512, w_scale=ws)
    ref = O.astype(np.float64) @ W.astype(np.float64).T
    assert np.abs(C.cpu().numpy()[:M] - ref).max() < 3e-5


def test_attention_random_ragged_shapes(ops):
    """Seeded random segment lengths up to 700 queries / keys (several 256-query workgroups, partial last key tiles, single
    rows) through the default dispatch: the BF16-split kernel when the longest query segment exceeds 64, the fp32 one below."""
    rng = np.random.default_rng(2024)
    for trial in range(6):
        B = int(rng.integers(1, 5))
        q_lens = [int(x) for x in rng.integers(1, 700 if trial % 2 == 0 else 60, B)]
        kv_lens = [int(x) for x in rng.integers(1, 700, B)]
        _attn_case(ops, q_lens, kv_lens, 100 + trial)
    _attn_case(ops, [257, 513], [31, 97], 77, spike=True)          # large scores on few keys: the lazy-rescale path


def test_attention_large_score_range(ops):
    """Scores spanning hundreds of units (Q and K scaled up): the lazy rescale must still move the reference maximum."""
    rng = np.random.default_rng(31)
    H, dk = 4, 128
    q_lens, kv_lens = [300], [400]
    Q = (rng.standard_normal((300, H * dk)) * 6).astype(np.float32)
    K = (rng.standard_normal((400, H * dk)) * 6).astype(np.float32)
    K[np.arange(0, 400, 7)] *= np.linspace(0.2, 3.0, len(range(0, 400, 7)))[:, None].astype(np.float32)     # growing maxima
    V = rng.standard_normal((400, H * dk)).astype(np.float32)
    z = np.zeros(1, np.int32)
    O = ops.attention(dev(Q), dev(K), dev(V), dev(z), dev(np.asarray(q_lens, np.int32)), dev(z), dev(np.asarray(kv_lens, np.int32)),
                      H, dk ** -0.5).cpu().numpy()
    ref = P.mha(Q.astype(np.float64), K.astype(np.float64), V.astype(np.float64), H)
    assert np.isfinite(O).all()
    # scores of magnitude ~500: their fp32 rounding (3e-5) goes straight into the exponent — the fp32-MFMA kernel measures 1.0e-4
    # here, the BF16-split kernel 7.4e-5
    assert np.abs(O - ref).max() < 3e-4, np.abs(O - ref).max()


def test_cif_bit_exact_against_oracle(ops):
    rng = np.random.default_rng(17)
    lens = [1, 5, 83, 500, 0, 9]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    M = sum(lens)
    # D = 320 / 512: cif_kernel<1>; D = 516: cif_kernel<2> with four channels in its second slot
    for D in (320, 512, 516):
        hidden = rng.standard_normal((M, D)).astype(np.float32)
        # the second set: multiples of 1/16 in [0, 1], whose running sums are exact in fp32, so that alpha + integrate == threshold
        # happens (uniform alphas never meet the threshold) and an alpha of 1.0 fires on its own frame
        for alphas in (rng.uniform(0, 0.7, M).astype(np.float32), (rng.integers(0, 17, M) / 16.0).astype(np.float32)):
            stage, nf, tn = ops.cif(dev(hidden), dev(alphas), dev(off), dev(np.asarray(lens, np.int32)), 1.0, 0.45)
            stage, nf, tn = stage.cpu().numpy(), nf.cpu().numpy(), tn.cpu().numpy()
            for b, (o, L) in enumerate(zip(off, lens)):
                if L == 0:
                    assert nf[b] == 0 and tn[b] == 0
                    continue
                h = np.concatenate([hidden[o:o + L], np.zeros((1, D), np.float32)])
                a = np.concatenate([alphas[o:o + L], np.asarray([0.45], np.float32)])
                emb, _ = P.cif(h, a, 1.0)
                assert nf[b] == emb.shape[0]
                assert tn[b] == int(np.floor(np.cumsum(a, dtype=np.float32)[-1]))
                # same operations in the same order with contraction off: bit-exact
                assert np.array_equal(stage[o + b:o + b + nf[b]], emb)


def test_logsoftmax_argmax_first_max_wins(ops):
    rng = np.random.default_rng(19)
    V, Vp = 1003, 1024
    x = rng.standard_normal((50, Vp)).astype(np.float32)
    x[3, 700] = x[3, 20] = 9.0          # tie -> index 20 (util.cpp:63-74 strict '>')
    x[4, :V] = -5.0                     # all equal -> index 0
    x[5, V:] = 100.0                    # pad columns must be ignored
    logp, ids = ops.logsoftmax_argmax(dev(x), V=V)
    logp, ids = logp.cpu().numpy(), ids.cpu().numpy()
    ref_ids = x[:, :V].argmax(-1)
    assert np.array_equal(ids, ref_ids) and ids[3] == 20 and ids[4] == 0
    z = x[:, :V] - x[:, :V].max(-1, keepdims=True)
    ref = z - np.log(np.exp(z).sum(-1, keepdims=True))
    assert np.abs(logp - ref).max() < 1e-5
    # ids only (the greedy path of the offline forward): one pass, 16-byte loads where V % 4 == 0 — same first-maximum rule
    for V2 in (1003, 1004, 8):
        y = rng.standard_normal((37, Vp)).astype(np.float32)
        y[3, 701] = y[3, 22] = 9.0
        y[4, :V2] = -5.0
        y[5, V2:] = 100.0
        y[6, 3] = y[6, 2] = y[6, 1] = 7.5       # a tie inside one 16-byte load
        _, ids2 = ops.logsoftmax_argmax(dev(y), V=V2, want_logp=False)
        assert np.array_equal(ids2.cpu().numpy(), y[:, :V2].argmax(-1))


def test_gemm_random_shapes_all_kernels(ops):
    """Seeded random (M, N, K) incl. ragged edges, every kernel kind with bounds checks on: catches tile-edge mistakes that
    the fixed shapes above might miss."""
    rng = np.random.default_rng(123)
    for trial in range(24):
        M = int(rng.integers(1, 700))
        N = int(rng.integers(1, 900))
        K = 32 * int(rng.integers(1, 20))
        A = rng.standard_normal((M, K)).astype(np.float32)
        W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
        bias = rng.standard_normal(N).astype(np.float32)
        R1 = rng.standard_normal((M, N)).astype(np.float32)
        Np = (N + 127) // 128 * 128
        dA, dW = dev(pad_rows(A)), dev(pad_rows(W))
        dbias = dev(np.concatenate([bias, np.zeros(Np - N, np.float32)]))
        dR1 = dev(np.pad(pad_rows(R1), ((0, 0), (0, Np - N))))
        ref = np.maximum(A @ W.T + bias + R1, 0)
        for kind in (1, 2, 3, 4, 5, 7, 8, 9, 10):
            C = ops.gemm_f32(dA, dW, bias=dbias, R1=dR1, relu=True, M=M, N=N, guard=True, kind=kind).cpu().numpy()
            assert np.abs(C[:M, :N] - ref).max() < 3e-5 * max(1.0, np.sqrt(K / 512)), (M, N, K, kind)


def test_gemm_bf16_split_is_fp32_grade(ops):
    """The BF16-matrix-core kernel (exact 3-way operand split, six MFMAs per block) against an fp64 reference: not further
    away than the fp32 MFMA kernel, over a wide dynamic range of operand magnitudes (the split keeps fp32's exponent range),
    and exact on integer data."""
    rng = np.random.default_rng(5)
    M, N, K = 700, 384, 1024
    scale_a = np.exp2(rng.integers(-40, 40, (M, 1))).astype(np.float32)       # rows of very different magnitude
    A = (rng.standard_normal((M, K)) * scale_a).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    dA, dW = dev(pad_rows(A)), dev(pad_rows(W))
    ref = A.astype(np.float64) @ W.astype(np.float64).T
    norm = np.sqrt((A.astype(np.float64) ** 2).sum(1, keepdims=True)) * np.sqrt((W.astype(np.float64) ** 2).sum(1))[None, :]
    err = {}
    for kind in (1, 4, 5, 7):
        C = ops.gemm_f32(dA, dW, M=M, N=N, guard=True, kind=kind).cpu().numpy()[:M, :N]
        err[kind] = float((np.abs(C - ref) / norm).max())
    assert err[4] <= 1.5 * err[1] + 1e-9 and err[5] <= 1.5 * err[1] + 1e-9 and err[7] <= 1.5 * err[1] + 1e-9, err
    assert err[4] < 5e-7 and err[5] < 5e-7 and err[7] < 5e-7, err
    Ai = rng.integers(-700, 700, (300, 32)).astype(np.float32)                 # 10-bit operands (two planes); sums < 2^24: exact
    Wi = rng.integers(-700, 700, (256, 32)).astype(np.float32)
    for kind in (4, 5, 7):
        C = ops.gemm_f32(dev(pad_rows(Ai)), dev(pad_rows(Wi)), M=300, N=256, guard=True, kind=kind).cpu().numpy()[:300, :256]
        assert np.array_equal(C, (Ai.astype(np.float64) @ Wi.astype(np.float64).T).astype(np.float32))


def test_gemm_f16_split_is_fp32_grade(ops):
    """The fp16 two-plane kernels (gemm_x3.hip: x = hi + lo in fp16, THREE products per block) against an fp64 reference, with
    the weight scale the model fixes per matrix at load (best_w_scale): the operands keep 22-23 significant bits, which is below
    what an fp32 accumulation chain of the same length commits — on rows of O(1) the error is that of the fp32 MFMA kernel
    (x 1.5).  Activations are staged unscaled: an ABSOLUTE floor of 2^-25 per element, so rows of small norm keep the absolute
    accuracy of O(1) rows, not their own relative one (second half).  One-plane integers come out exact."""
    rng = np.random.default_rng(15)
    M, N, K = 700, 384, 1024
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    A = rng.standard_normal((M, K)).astype(np.float32)
    dA, dW = dev(pad_rows(A)), dev(pad_rows(W))
    ref = A.astype(np.float64) @ W.astype(np.float64).T
    norm = np.sqrt((A.astype(np.float64) ** 2).sum(1, keepdims=True)) * np.sqrt((W.astype(np.float64) ** 2).sum(1))[None, :]
    err, rms = {}, {}
    for kind in (1, 4, 8, 9, 10):
        C = ops.gemm_f32(dA, dW, M=M, N=N, guard=True, kind=kind, w_scale="auto").cpu().numpy()[:M, :N]
        err[kind] = float((np.abs(C - ref) / norm).max())
        rms[kind] = float(np.sqrt((((C - ref) / norm) ** 2).mean()))
    for kind in (8, 9, 10):
        assert rms[kind] <= 1.5 * rms[1] + 1e-9 and err[kind] <= 1.5 * err[1] + 1e-9 and err[kind] < 5e-7, (err, rms)
    # unscaled weights of this magnitude (row norm 1, elements ~0.03) sit on the fp16 floor: still within 3 x the fp32 kernel
    C1 = ops.gemm_f32(dA, dW, M=M, N=N, guard=True, kind=9).cpu().numpy()[:M, :N]
    assert np.sqrt((((C1 - ref) / norm) ** 2).mean()) <= 3.0 * rms[1], rms
    # rows from 2^-7 to 2^7: the absolute error of a row stays what it is for an O(1) row (floor 2^-25 per element)
    scale_a = np.exp2(rng.integers(-7, 8, (M, 1))).astype(np.float32)
    A2 = (A * scale_a).astype(np.float32)
    ref2 = A2.astype(np.float64) @ W.astype(np.float64).T
    wn = np.sqrt((W.astype(np.float64) ** 2).sum(1))[None, :]
    for kind in (8, 9, 10):
        C = ops.gemm_f32(dev(pad_rows(A2)), dW, M=M, N=N, guard=True, kind=kind, w_scale="auto").cpu().numpy()[:M, :N]
        abs_err = np.abs(C - ref2) / wn
        big = (scale_a[:, 0] >= 1)
        assert (abs_err[big] / (np.sqrt(K) * scale_a[big])).max() < 5e-7             # O(1) and larger rows: relative to their norm
        assert abs_err[~big].max() < 5e-7 * np.sqrt(K), abs_err[~big].max()          # smaller rows: the absolute bound of an O(1) row
    Ai = rng.integers(-1000, 1000, (300, 32)).astype(np.float32)               # 10-bit operands: one plane; sums < 2^24: exact
    Wi = rng.integers(-1000, 1000, (256, 32)).astype(np.float32)
    for kind in (8, 9, 10):
        for ws in (None, "auto"):
            C = ops.gemm_f32(dev(pad_rows(Ai)), dev(pad_rows(Wi)), M=300, N=256, guard=True, kind=kind, w_scale=ws).cpu().numpy()[:300, :256]
            assert np.array_equal(C, (Ai.astype(np.float64) @ Wi.astype(np.float64).T).astype(np.float32))


def test_gemm_f16_split_stated_domain(ops):
    """Where the fp16 form stops being an fp32 GEMM, pinned (the scaling note at the top of gemm_x3.hip):
      * |a| >= 65504 (or +-Inf): the high plane saturates and the low plane overflows — EVERY output of that row is Inf or NaN,
        a loud failure (the bf16 form is exact for any finite magnitude and gives NaN rows for Inf); NaN stays NaN; other rows
        are untouched;
      * small magnitudes: absolute floor 2^-25 per element: rows of magnitude 2^-10 keep ~14 bits, rows at 2^-4 are fp32-grade.
    LayerNorm-ed activations, residual streams and weights of O(1e-3 .. 1e3) are inside; callers outside it use PFHIP_GEMM_X3=0."""
    rng = np.random.default_rng(16)
    M, N, K = 256, 256, 512
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    A[3, 17] = 1e6
    A[9, 100] = -np.inf
    A[40, 5] = np.nan
    ref = A.astype(np.float64) @ W.astype(np.float64).T
    for kind in (8, 9, 10):
        C = ops.gemm_f32(dev(pad_rows(A)), dev(pad_rows(W)), M=M, N=N, guard=True, kind=kind, w_scale="auto").cpu().numpy()[:M, :N]
        # the high plane saturates at 65504, the low plane (round to nearest) overflows: the row fails LOUDLY (Inf / NaN)
        assert not np.isfinite(C[3]).any() and not np.isfinite(C[9]).any() and np.isnan(C[40]).all(), kind
        ok = [r for r in range(M) if r not in (3, 9, 40)]
        assert np.isfinite(C[ok]).all() and np.abs(C[ok] - ref[ok]).max() < 3e-5, kind
    A2 = rng.standard_normal((M, K)).astype(np.float32)
    scale = np.ones((M, 1), np.float32)
    scale[:128] = np.float32(2.0 ** -4)
    scale[128:] = np.float32(2.0 ** -10)
    A2 = (A2 * scale).astype(np.float32)
    ref2 = A2.astype(np.float64) @ W.astype(np.float64).T
    norm = np.sqrt((A2.astype(np.float64) ** 2).sum(1, keepdims=True)) * np.sqrt((W.astype(np.float64) ** 2).sum(1))[None, :]
    for kind in (8, 9, 10):
        C = ops.gemm_f32(dev(pad_rows(A2)), dev(pad_rows(W)), M=M, N=N, guard=True, kind=kind, w_scale="auto").cpu().numpy()[:M, :N]
        rel = np.abs(C - ref2) / norm
        assert rel[:128].max() < 5e-7, (kind, rel[:128].max())
        assert rel[128:].max() < 2.0 ** -13, (kind, rel[128:].max())


@pytest.mark.parametrize("M,N,K,relu", [(300, 512, 512, False), (1000, 256, 2048, True), (128, 128, 16, False), (257, 1536, 576, True)])
def test_gemm_on_pre_split_operands(ops, M, N, K, relu):
    """gemm_p3.hip: both operands arrive as fp16 plane images (split once: weights at load, activations by their producer), the
    K-loop is LDS-DMA + fragment reads + three MFMAs per block.  fp32 output and plane output (decoded on the host) against fp64,
    at the accuracy of the in-loop-split kernels; the images themselves round-trip to 22+ bits."""
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    R1 = rng.standard_normal((M, N)).astype(np.float32)
    ws = ops.best_w_scale(float(np.abs(W).max()))
    a_img = ops.split_planes(dev(A))
    w_img = ops.split_planes(dev(W), scale=ws)
    back = ops.planes_to_float(a_img[0], a_img[1], a_img[2], K)[:M]
    assert np.abs(back - A).max() <= 2.0 ** -22 * np.abs(A).max() + 2.0 ** -24
    assert np.abs(ops.planes_to_float(a_img[0], a_img[1], a_img[2], K)[M:]).max() == 0 if a_img[2] > M else True
    ref = A.astype(np.float64) @ W.astype(np.float64).T + bias + R1
    if relu:
        ref = np.maximum(ref, 0)
    Mp = (M + 127) // 128 * 128
    dR1 = dev(np.pad(R1, ((0, Mp - M), (0, 0))))
    tol = 3e-5 * max(1.0, np.sqrt(K / 512))
    C, P = ops.gemm_p3(a_img, w_img, M, N, K, w_scale=ws, bias=dev(bias), R1=dR1, relu=relu, want_c=True, want_planes=True)
    assert np.abs(C.cpu().numpy()[:M] - ref).max() < tol
    pl = ops.planes_to_float(P[0], P[1], P[2], N)[:M]
    assert np.abs(pl - ref).max() < tol + 2.0 ** -21 * np.abs(ref).max()
    C1, _ = ops.gemm_p3(a_img, w_img, M, N, K, w_scale=ws, bias=dev(bias), R1=dR1, relu=relu, want_c=True, want_planes=False)
    assert np.array_equal(C1.cpu().numpy()[:M], C.cpu().numpy()[:M])
    # both tile heights (64 x 128: three workgroups per CU for small grids; 128 x 128), every output form: bit-identical
    for tr in (64, 128, 256):
        Ct, Pt = ops.gemm_p3(a_img, w_img, M, N, K, w_scale=ws, bias=dev(bias), R1=dR1, relu=relu, want_c=True, want_planes=True, tile_rows=tr)
        assert np.array_equal(Ct.cpu().numpy()[:M], C.cpu().numpy()[:M]), tr
        assert np.array_equal(ops.planes_to_float(Pt[0], Pt[1], Pt[2], N)[:M], pl), tr
        _, Pt2 = ops.gemm_p3(a_img, w_img, M, N, K, w_scale=ws, bias=dev(bias), relu=relu, want_c=False, want_planes=True, tile_rows=tr)
        Ct2, _ = ops.gemm_p3(a_img, w_img, M, N, K, w_scale=ws, bias=dev(bias), relu=relu, want_c=True, want_planes=False, tile_rows=tr)
        assert np.abs(ops.planes_to_float(Pt2[0], Pt2[1], Pt2[2], N)[:M] - Ct2.cpu().numpy()[:M]).max() <= 2.0 ** -21 * max(1.0, np.abs(ref).max()), tr
    ref2 = A.astype(np.float64) @ W.astype(np.float64).T + bias              # planes only: no residual (FFN1's form)
    if relu:
        ref2 = np.maximum(ref2, 0)
    _, P2 = ops.gemm_p3(a_img, w_img, M, N, K, w_scale=ws, bias=dev(bias), relu=relu, want_c=False, want_planes=True)
    assert np.abs(ops.planes_to_float(P2[0], P2[1], P2[2], N)[:M] - ref2).max() < tol + 2.0 ** -21 * np.abs(ref2).max()
    # chaining: the plane output of one GEMM is the A operand of the next
    if N % 16 == 0 and N <= 2048:
        W2 = (rng.standard_normal((128, N)) / np.sqrt(N)).astype(np.float32)
        ws2 = ops.best_w_scale(float(np.abs(W2).max()))
        C3, _ = ops.gemm_p3(P2, ops.split_planes(dev(W2), scale=ws2), M, 128, N, w_scale=ws2)
        assert np.abs(C3.cpu().numpy()[:M] - ref2 @ W2.astype(np.float64).T).max() < 2 * tol * max(1.0, np.sqrt(N / 512)) * max(1.0, np.abs(ref2).max() / 4)


def test_three_stage_tile_is_bit_identical(ops, monkeypatch):
    """gemm_p3_128r3_kernel (ring of three stages, three workgroups per CU, the C tile out in two 64-row halves; picked by itself for
    grids beyond 1536 tiles, PFHIP_P3_R3=1 forces it): same MFMA order and epilogue arithmetic as the four-stage kernel — every output
    form must match it bit for bit, ragged M and a K that leaves a tail of the six-step pattern included."""
    rng = np.random.default_rng(77)
    for M, N, K, ln in ((1000, 512, 512, False), (777, 1536, 512, True), (300, 256, 80, False), (2050, 512, 2048, False)):
        A = rng.standard_normal((M, K)).astype(np.float32)
        W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
        bias = rng.standard_normal(N).astype(np.float32)
        R1 = rng.standard_normal(((M + 127) // 128 * 128, N)).astype(np.float32)
        ws = ops.best_w_scale(float(np.abs(W).max()))
        a_img, w_img = ops.split_planes(dev(A)), ops.split_planes(dev(W), scale=ws)
        kw = {}
        if ln:
            Mp = (M + 127) // 128 * 128
            stats = np.zeros((Mp, 4, 2), np.float32)
            t = A.reshape(M, 4, 128).astype(np.float64)
            stats[:M, :, 0] = t.mean(2)
            stats[:M, :, 1] = ((t - t.mean(2, keepdims=True)) ** 2).sum(2)
            kw = dict(ln_stats=dev(stats), ln_tiles=4, ln_colsum=dev(W.astype(np.float64).sum(1).astype(np.float32)))
        outs = []
        for r3 in ("0", "1"):
            monkeypatch.setenv("PFHIP_P3_R3", r3)
            st = torch.zeros(((M + 127) // 128 * 128, N // 128, 2), device="cuda")
            C, P = ops.gemm_p3(a_img, w_img, M, N, K, w_scale=ws, bias=dev(bias), R1=None if ln else dev(R1), relu=ln, want_c=True,
                               want_planes=True, stats_out=None if ln else st, tile_rows=128, **kw)
            _, P2 = ops.gemm_p3(a_img, w_img, M, N, K, w_scale=ws, bias=dev(bias), relu=True, want_c=False, want_planes=True, tile_rows=128, **kw)
            outs.append((C.cpu().numpy()[:M], P[0].cpu().numpy(), P[1].cpu().numpy(), P2[0].cpu().numpy(), P2[1].cpu().numpy(), st.cpu().numpy()[:M]))
        for x, y in zip(*outs):
            assert np.array_equal(x, y)
        monkeypatch.delenv("PFHIP_P3_R3")
        if not ln:
            ref = A.astype(np.float64) @ W.astype(np.float64).T + bias + R1[:M]
            assert np.abs(outs[1][0] - ref).max() < 3e-5 * max(1.0, np.sqrt(K / 512))


def test_plane_operand_tiles_agree_on_random_shapes(ops, monkeypatch):
    """Twelve random (M, N, K) — ragged row counts, K from one K-step to 130, every tail of the four- and six-step loop patterns — through
    the 64-, 128- (four- and three-stage) and 256-row tiles of gemm_p3.hip: all five C / plane outputs bit-identical, and the fp32
    result within the two-plane bound of the fp64 product."""
    rng = np.random.default_rng(4242)
    for case in range(12):
        M = int(rng.integers(1, 1400))
        N = 128 * int(rng.integers(1, 5))
        K = 16 * int(rng.integers(1, 131))
        A = rng.standard_normal((M, K)).astype(np.float32)
        W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
        bias = rng.standard_normal(N).astype(np.float32)
        Mp = (M + 127) // 128 * 128
        R1 = rng.standard_normal((Mp, N)).astype(np.float32)
        ws = ops.best_w_scale(float(np.abs(W).max()))
        a_img, w_img = ops.split_planes(dev(A)), ops.split_planes(dev(W), scale=ws)
        relu = bool(case & 1)
        outs = []
        for tr, r3 in ((128, "0"), (128, "1"), (64, "0"), (256, "0")):
            if tr == 256 and Mp < 256:
                continue
            monkeypatch.setenv("PFHIP_P3_R3", r3)
            st = torch.zeros((Mp, N // 128, 2), device="cuda")
            C, P = ops.gemm_p3(a_img, w_img, M, N, K, w_scale=ws, bias=dev(bias), R1=dev(R1), relu=relu, want_c=True, want_planes=True,
                               stats_out=st, tile_rows=tr)
            outs.append((tr, r3, C.cpu().numpy()[:M], ops.planes_to_float(P[0], P[1], P[2], N)[:M], st.cpu().numpy()[:M]))
        monkeypatch.delenv("PFHIP_P3_R3")
        for tr, r3, C, Pf, st in outs[1:]:
            assert np.array_equal(C, outs[0][2]), (case, M, N, K, tr, r3)
            assert np.array_equal(Pf, outs[0][3]), (case, M, N, K, tr, r3)
            assert np.array_equal(st, outs[0][4]), (case, M, N, K, tr, r3)
        ref = A.astype(np.float64) @ W.astype(np.float64).T + bias + R1[:M]
        if relu:
            ref = np.maximum(ref, 0)
        assert np.abs(outs[0][2] - ref).max() < 3e-5 * max(1.0, np.sqrt(K / 512)), (case, M, N, K)


def test_gemm_on_pre_split_operands_refuses_bad_shapes(ops):
    """The operator checks on the host what its grid and DMA assume; a refused call launches nothing."""
    A = dev(np.ones((128, 64), np.float32))
    W = dev(np.ones((128, 64), np.float32))
    a_img, w_img = ops.split_planes(A), ops.split_planes(W)
    for kw in (dict(M=129, N=128, K=64),       # more rows than the A image holds
               dict(M=128, N=256, K=64),       # more columns than the W image holds
               dict(M=128, N=128, K=72),       # K not a multiple of the 16-deep step
               dict(M=128, N=96, K=64)):       # N not a multiple of the tile
        with pytest.raises(RuntimeError):
            ops.gemm_p3(a_img, w_img, kw["M"], kw["N"], kw["K"])
    with pytest.raises(RuntimeError):
        ops.gemm_p3(a_img, w_img, 128, 128, 64, w_scale=0.0)
    C, _ = ops.gemm_p3(a_img, w_img, 128, 128, 64)
    assert np.array_equal(C.cpu().numpy(), np.full((128, 128), 64.0, np.float32))


def test_gemm_bf16_split_stated_domain(ops):
    """Where the three-plane split (gemm_x6.hip: rest(x) = x - top16(x)) stops being an fp32 GEMM, pinned:
      * a non-finite operand: Inf - Inf = NaN in the second plane, so EVERY output of that row is NaN (an fp32 GEMM would carry
        +-Inf through, NaN only where signs cancel); rows without non-finite operands are untouched;
      * operands below 2^-110: the third plane (2^-16 of the operand) falls into bf16's denormal range and the matrix cores
        flush it — the result keeps ~16 significant bits instead of 24.  Down to 2^-100 the split is exact.
    Neither is reachable from LayerNorm-ed activations and finite weights; this test states the domain of the precision claim."""
    rng = np.random.default_rng(6)
    M, N, K = 256, 256, 512
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    A[3, 17] = np.inf
    A[9, 100] = -np.inf
    A[40, 5] = np.nan
    ref = A.astype(np.float64) @ W.astype(np.float64).T
    for kind in (4, 5, 7):
        C = ops.gemm_f32(dev(pad_rows(A)), dev(pad_rows(W)), M=M, N=N, guard=True, kind=kind).cpu().numpy()[:M, :N]
        for r in (3, 9, 40):
            assert np.isnan(C[r]).all(), (kind, r)                    # the fp32-MFMA kernel gives +-Inf in rows 3 and 9
        ok = [r for r in range(M) if r not in (3, 9, 40)]
        assert np.isfinite(C[ok]).all() and np.abs(C[ok] - ref[ok]).max() < 3e-5, kind
    Cf = ops.gemm_f32(dev(pad_rows(A)), dev(pad_rows(W)), M=M, N=N, guard=True, kind=1).cpu().numpy()[:M, :N]
    assert np.isinf(Cf[3]).all() and np.isinf(Cf[9]).all() and np.isnan(Cf[40]).all()
    # magnitude floor: rows scaled by 2^-100 are still fp32-grade, rows at 2^-118 keep at least 14 bits
    A2 = rng.standard_normal((M, K)).astype(np.float32)
    scale = np.ones((M, 1), np.float32)
    scale[:128] = np.float32(2.0 ** -100)
    scale[128:] = np.float32(2.0 ** -118)
    A2 = (A2 * scale).astype(np.float32)
    ref2 = A2.astype(np.float64) @ W.astype(np.float64).T
    norm = np.sqrt((A2.astype(np.float64) ** 2).sum(1, keepdims=True)) * np.sqrt((W.astype(np.float64) ** 2).sum(1))[None, :]
    for kind in (4, 5, 7):
        C = ops.gemm_f32(dev(pad_rows(A2)), dev(pad_rows(W)), M=M, N=N, guard=True, kind=kind).cpu().numpy()[:M, :N]
        rel = np.abs(C - ref2) / norm
        assert rel[:128].max() < 5e-7, (kind, rel[:128].max())
        assert rel[128:].max() < 2.0 ** -14, (kind, rel[128:].max())


def test_fp32_mfma_kernels_behind_the_opt_out_knobs():
    """PFHIP_ATT_X6=0 / PFHIP_GEMM_X6=0 keep everything on the fp32-MFMA kernels (the knobs are read once per process, hence
    a child process): the d_k = 128 attention cases above and the full-size oracle comparison must pass there too."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PFHIP_ATT_X6="0", PFHIP_GEMM_X6="0")
    out = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "tests/test_gpu_ops.py", "tests/test_gpu_forward.py",
                          "-k", "attention_self or attention_cross or attention_rescale or full_size_batch_matches_oracle"],
                         cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout


def test_bf16_six_product_forms_behind_their_knobs():
    """PFHIP_GEMM_X3=0 / PFHIP_ATT_X3=0 keep the large launches on the three-plane bf16 kernels (gemm_x6.hip, attention_x6.hip:
    fp32's exponent range) — the form every round-2 result was measured on; the attention cases and the model-level comparisons
    with the oracle must pass there too (child process: the knobs are read once)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PFHIP_ATT_X3="0", PFHIP_GEMM_X3="0")
    out = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "tests/test_gpu_ops.py", "tests/test_gpu_forward.py",
                          "-k", "attention_self or attention_cross or attention_rescale or full_size_batch_matches_oracle or layernorm_folded"],
                         cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout


@pytest.mark.parametrize("M,N,K,D,ln,fsmn", [(20, 1536, 512, 512, True, False), (20, 1536, 576, 560, True, False), (20, 512, 512, 512, False, True),
                                              (1, 512, 2048, 2048, True, False), (7, 2048, 512, 512, True, False), (32, 512, 2048, 2048, False, False),
                                              (13, 8404, 512, 512, True, False), (20, 16384, 512, 512, False, False), (9, 1003, 512, 512, True, False)])
def test_fused_ln_gemm_one_window(ops, M, N, K, D, ln, fsmn):
    """stream_fused.hip: LayerNorm (non-trivial gamma / beta, width D <= K) -> GEMM (+bias, +residual, ReLU) (+ the SAN-M FSMN
    memory of a value matrix over the M rows) in ONE launch, against fp64; both forms (vector-ALU GEMV for N <= 4096, MFMA for the
    vocabulary-sized ones)."""
    rng = np.random.default_rng(M * 1000 + N)
    Np = (N + 127) // 128 * 128
    X = np.zeros((32, K), np.float32)
    X[:M, :D] = (rng.standard_normal((M, D)) * 3 + 1.5).astype(np.float32)
    W = np.zeros((Np + 128, K), np.float32)
    W[:N, :D] = (rng.standard_normal((N, D)) / np.sqrt(D)).astype(np.float32)
    g = (rng.random(K) + 0.5).astype(np.float32)
    b = (rng.standard_normal(K) * 0.2).astype(np.float32)
    bias = np.zeros(Np, np.float32); bias[:N] = rng.standard_normal(N)
    R = rng.standard_normal((32, Np)).astype(np.float32)
    V = rng.standard_normal((32, Np)).astype(np.float32)
    fw = (rng.standard_normal((Np, 11)) / 3).astype(np.float32)
    xd = X[:M, :D].astype(np.float64)
    if ln:
        xd = (xd - xd.mean(1, keepdims=True)) / np.sqrt(xd.var(1, keepdims=True) + 1e-12) * g[:D] + b[:D]
    ref = xd @ W[:N, :D].astype(np.float64).T + bias[:N] + R[:M, :N]
    if fsmn:
        mem = V[:M, :N].astype(np.float64).copy()
        for t in range(M):
            for j in range(11):
                s = t + j - 5
                if 0 <= s < M:
                    mem[t] += fw[:N, j] * V[s, :N]
        ref = ref + mem
    ref = np.maximum(ref, 0)
    out = ops.fused_ln_gemm(dev(X), dev(W), M, N, g=dev(g) if ln else None, b=dev(b) if ln else None, D=D, bias=dev(bias), R1=dev(R),
                            fsmn_v=dev(V) if fsmn else None, fsmn_w=dev(fw) if fsmn else None, relu=True).cpu().numpy()
    assert np.abs(out[:M, :N] - ref).max() < 5e-5 * np.sqrt(K / 512)
    assert not out[M:].any()                 # rows beyond M are not written


@pytest.mark.parametrize("M,N,K,ln,fsmn", [(20, 1536, 512, True, False), (20, 512, 512, False, True), (20, 2048, 512, True, False),
                                           (20, 512, 2048, False, False), (1, 512, 2048, True, False), (7, 2048, 512, True, False),
                                           (8, 512, 512, True, False), (13, 16384, 512, False, False), (3, 512, 512, False, True)])
def test_fused_gemv_one_trip(ops, M, N, K, ln, fsmn):
    """stream_fused.hip, one-trip form: LayerNorm applied ALGEBRAICALLY on gamma/beta-folded weights (rstd * (x W'^T - mean * colsum)
    + b', statistics merged with Chan's formula from the same loaded values) -> GEMM (+bias, +residual, ReLU) (+ FSMN memory), against
    the explicit two-pass LayerNorm in fp64.  Rows with a mean several times their spread, gamma in [0.5, 1.5], beta ~ 0.2."""
    import torch
    rng = np.random.default_rng(M * 1000 + N + K)
    X = np.zeros((32, K), np.float32)
    X[:M] = (rng.standard_normal((M, K)) * 3 + 4.5).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    g = (rng.random(K) + 0.5).astype(np.float32)
    b = (rng.standard_normal(K) * 0.2).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    R = rng.standard_normal((32, N)).astype(np.float32)
    V = rng.standard_normal((32, N)).astype(np.float32)
    fw = (rng.standard_normal((N, 11)) / 3).astype(np.float32)
    xd = X[:M].astype(np.float64)
    if ln:
        xd = (xd - xd.mean(1, keepdims=True)) / np.sqrt(xd.var(1, keepdims=True) + 1e-12) * g + b
    ref = xd @ W.astype(np.float64).T + bias + R[:M]
    if fsmn:
        mem = V[:M].astype(np.float64).copy()
        for t in range(M):
            for j in range(11):
                s = t + j - 5
                if 0 <= s < M:
                    mem[t] += fw[:, j] * V[s]
        ref = ref + mem
    ref = np.maximum(ref, 0)
    Wd, bd, cs = dev(W), dev(bias), None
    if ln:
        Wd, bd, cs = ops.fold_layernorm(Wd, bd, dev(g), dev(b))
    out = torch.zeros((32, N), dtype=torch.float32, device="cuda")
    ops.fused_gemv_1trip(dev(X), Wd, M, N, bias=bd, ln_colsum=cs, R1=dev(R), fsmn_v=dev(V) if fsmn else None,
                         fsmn_w=dev(fw) if fsmn else None, relu=True, out=out)
    out = out.cpu().numpy()
    # the algebraic form subtracts mean * colsum from the raw dot product: its rounding scales with sqrt(mean^2 + var) / std (~1.8 here)
    assert np.abs(out[:M] - ref).max() < 1e-4 * np.sqrt(K / 512)
    assert not out[M:].any()                 # rows beyond M are not written


def test_fused_gemv_one_trip_rejects_other_shapes(ops):
    import torch
    X = torch.zeros((32, 576), device="cuda"); W = torch.zeros((1536, 576), device="cuda")
    with pytest.raises(Exception):
        ops.fused_gemv_1trip(X, W, 20, 1536)          # K = 576: not a whole number of k-blocks
    X = torch.zeros((32, 512), device="cuda"); W = torch.zeros((512, 512), device="cuda")
    with pytest.raises(Exception):
        ops.fused_gemv_1trip(X, W, 21, 512)           # more rows than a window's lanes hold


@pytest.mark.parametrize("Lq,Lk,H", [(20, 20, 4), (1, 20, 4), (7, 20, 4), (32, 32, 4), (10, 10, 4), (3, 1, 2), (20, 13, 4)])
def test_window_attention(ops, Lq, Lk, H):
    """stream_fused.hip window_attention_kernel (one streaming window, d_k = 128) against softmax(QK^T)V in fp64; Q / K / V as column
    blocks of one row-major buffer, as the streaming encoder hands them over; large score range."""
    import torch
    rng = np.random.default_rng(Lq * 100 + Lk)
    d = H * 128
    qkv = (rng.standard_normal((32, 3 * d)) * 2.0).astype(np.float32)
    t = dev(qkv)
    out = ops.window_attention(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], Lq, Lk, H, 128 ** -0.5).cpu().numpy()
    for h in range(H):
        q = qkv[:Lq, h * 128:(h + 1) * 128].astype(np.float64)
        k = qkv[:Lk, d + h * 128:d + (h + 1) * 128].astype(np.float64)
        v = qkv[:Lk, 2 * d + h * 128:2 * d + (h + 1) * 128].astype(np.float64)
        sc = q @ k.T * 128 ** -0.5
        p = np.exp(sc - sc.max(1, keepdims=True)); p /= p.sum(1, keepdims=True)
        assert np.abs(out[:Lq, h * 128:(h + 1) * 128] - p @ v).max() < 2e-5
    assert not out[Lq:].any()
    with pytest.raises(Exception):
        ops.window_attention(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], 33, 20, H, 1.0)


@pytest.mark.parametrize("Lq,Lk,fsmn", [(20, 20, True), (1, 20, False), (7, 20, False), (10, 10, True), (20, 13, False), (3, 32, False)])
def test_fused_attention_and_projection(ops, Lq, Lk, fsmn):
    """stream_fused.hip fused_att_out_kernel: the window's attention (4 heads of 128) and the projection of its context (+bias,
    +residual, + FSMN memory of the value block) in one launch, against fp64."""
    import torch
    rng = np.random.default_rng(Lq * 100 + Lk + 7)
    H, d, N = 4, 512, 512
    qkv = (rng.standard_normal((32, 3 * d)) * 1.5).astype(np.float32)
    W = (rng.standard_normal((N, d)) / np.sqrt(d)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    R = rng.standard_normal((32, N)).astype(np.float32)
    fw = (rng.standard_normal((N, 11)) / 3).astype(np.float32)
    ctx = np.zeros((Lq, d))
    for h in range(H):
        q = qkv[:Lq, h * 128:(h + 1) * 128].astype(np.float64)
        k = qkv[:Lk, d + h * 128:d + (h + 1) * 128].astype(np.float64)
        v = qkv[:Lk, 2 * d + h * 128:2 * d + (h + 1) * 128].astype(np.float64)
        sc = q @ k.T * 128 ** -0.5
        p = np.exp(sc - sc.max(1, keepdims=True)); p /= p.sum(1, keepdims=True)
        ctx[:, h * 128:(h + 1) * 128] = p @ v
    ref = ctx @ W.astype(np.float64).T + bias + R[:Lq]
    if fsmn:
        V = qkv[:, 2 * d:].astype(np.float64)
        mem = V[:Lq].copy()
        for t in range(Lq):
            for j in range(11):
                s = t + j - 5
                if 0 <= s < Lq:
                    mem[t] += fw[:, j] * V[s]
        ref = ref + mem
    t = dev(qkv)
    out = ops.fused_att_out(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], Lq, Lk, H, 128 ** -0.5, dev(W), bias=dev(bias), R1=dev(R),
                            fsmn_v=t[:, 2 * d:] if fsmn else None, fsmn_w=dev(fw) if fsmn else None).cpu().numpy()
    assert np.abs(out[:Lq] - ref).max() < 5e-5
    assert not out[Lq:].any()
    with pytest.raises(Exception):
        ops.fused_att_out(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], 21, 20, H, 1.0, dev(W))


def _integer_epilogue_case(M, N, K, seed):
    """Integer-valued operands for test_split_gemm_epilogue_exact_on_integers and the int64 reference of
    relu(A W^T + bias + R1 + R2).  |A W^T| <= 16 K <= 1024 and the three addends are <= 64 each: every partial sum is an integer
    far below 2^24 (exact in the fp32 accumulator) and every operand has at most 3 significant bits (one fp16 / bf16 plane)."""
    rng = np.random.default_rng(seed)
    A = rng.integers(-4, 5, (M, K))
    W = rng.integers(-4, 5, (N, K))
    bias, R1, R2 = rng.integers(-64, 65, N), rng.integers(-64, 65, (M, N)), rng.integers(-64, 65, (M, N))
    ref = np.maximum(A @ W.T + bias[None, :] + R1 + R2, 0)
    # the reference itself is exactly representable: the same expression in float32 numpy gives the same integers
    f = lambda x: x.astype(np.float32)
    ref32 = np.maximum(f(A) @ f(W).T + f(bias)[None, :] + f(R1) + f(R2), np.float32(0))
    assert ref32.dtype == np.float32 and np.array_equal(ref32.astype(np.int64), ref)
    return f(A), f(W), f(bias), f(R1), f(R2), f(ref)


@pytest.mark.parametrize("kind", [4, 5, 7, 8, 9, 10])
def test_split_gemm_epilogue_exact_on_integers(ops, kind):
    """Every split form (bf16 six-product: kinds 4 / 5 / 7 = 256 / 128 / 64-row tile; fp16 three-product: 8 / 9 / 10) through the whole
    row epilogue at once — bias with a ragged last float4 group, R1, R2 and ReLU — on integers, where the result is exact: one
    and two row tiles of every tile height, one and two K-steps of the 32-deep kernel.  No tolerance."""
    for (M, N, K) in ((67, 130, 32), (129, 258, 64)):
        A, W, bias, R1, R2, ref = _integer_epilogue_case(M, N, K, 1000 * kind + M)
        pad_cols = lambda x: np.pad(x, ((0, 0), (0, -x.shape[1] % 128)))
        dR1, dR2 = dev(pad_rows(pad_cols(R1))), dev(pad_rows(pad_cols(R2)))
        C = ops.gemm_f32(dev(pad_rows(A)), dev(pad_rows(W)), bias=dev(np.pad(bias, (0, -N % 128))), R1=dR1, R2=dR2, relu=True, M=M, N=N,
                         guard=True, kind=kind, w_scale=1.0 if kind >= 8 else None).cpu().numpy()[:M, :N]
        assert np.array_equal(C, ref), (kind, M, N, K, int((C != ref).sum()), float(np.abs(C - ref).max()))
