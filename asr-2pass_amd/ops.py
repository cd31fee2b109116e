"""ctypes binding of the operator-level C ABI (include/pfhip_ops.h) over torch CUDA tensors.

torch is plumbing only here: it owns the device buffers and the stream; every op below runs the same
hand-written gfx950 kernel that pfhip_offline_forward launches.  No fallbacks: a missing library or a
non-CUDA tensor raises.
"""
from __future__ import annotations

import ctypes

import torch

from . import load_lib, PfhipError

_vp, _ci, _cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
_bound = False


def _lib():
    global _bound
    lib = load_lib()
    if not _bound:
        lib.pfhip_op_gemm_f32.argtypes = [_vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp]
        lib.pfhip_op_gemm_f32_kind.argtypes = [_vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _vp]
        lib.pfhip_op_fused_ln_gemm.argtypes = [_vp, _ci, _ci, _vp, _vp, _cf, _vp, _ci, _vp, _ci, _vp, _vp, _ci, _vp, _ci, _vp, _ci, _vp,
                                               _ci, _ci, _ci, _ci, _vp]
        lib.pfhip_op_fused_gemv_1trip.argtypes = [_vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _cf, _vp, _ci, _vp, _ci, _vp, _ci, _ci, _ci, _ci, _vp]
        lib.pfhip_op_window_attention.argtypes = [_vp, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _ci, _ci, _ci, _cf, _vp]
        lib.pfhip_op_window_attention_hd.argtypes = [_vp, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _ci, _ci, _ci, _cf, _ci, _vp]
        lib.pfhip_op_fused_att_out.argtypes = [_vp, _ci, _vp, _ci, _vp, _ci, _ci, _ci, _ci, _cf, _vp, _ci, _vp, _ci, _vp, _vp, _ci, _vp, _ci, _vp,
                                               _ci, _vp]
        lib.pfhip_op_layernorm.argtypes = [_vp, _ci, _vp, _ci, _vp, _vp, _ci, _ci, _ci, _cf, _vp]
        lib.pfhip_op_fsmn.argtypes = [_vp, _ci, _vp, _vp, _ci, _vp, _ci, _vp, _vp, _ci, _ci, _ci, _vp]
        lib.pfhip_op_attention.argtypes = [_vp, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _cf, _vp]
        lib.pfhip_op_attention_hd.argtypes = [_vp, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _cf, _ci, _vp]
        lib.pfhip_op_attention_dk.argtypes = [_vp, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _cf, _ci, _vp, _vp]
        lib.pfhip_op_cif.argtypes = [_vp, _ci, _vp, _vp, _vp, _ci, _ci, _cf, _cf, _vp, _vp, _vp, _vp]
        lib.pfhip_op_cif_fires.argtypes = [_vp, _ci, _vp, _vp, _vp, _ci, _ci, _cf, _cf, _vp, _vp, _vp, _vp, _vp]
        lib.pfhip_op_logsoftmax_argmax.argtypes = [_vp, _ci, _ci, _ci, _vp, _vp, _vp]
        lib.pfhip_op_logsoftmax_topk.argtypes = [_vp, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp]
        lib.pfhip_op_resample.argtypes = [_vp, _vp, _vp, _ci, _ci, _ci, _vp, _vp, _vp]
        if hasattr(lib, "pfhip_op_ctc_head"):          # (an older build loaded through PFHIP_LIB for A/B timing has none of these)
            lib.pfhip_op_ctc_head_workspace_bytes.restype = ctypes.c_size_t
            lib.pfhip_op_ctc_head_workspace_bytes.argtypes = [_ci, _ci]
            lib.pfhip_op_ctc_head.argtypes = [_vp, _ci, _vp, _ci, _vp, _cf, _ci, _ci, _ci, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]
            lib.pfhip_op_ctc_collapse.argtypes = [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp]
        if hasattr(lib, "pfhip_op_ctc_align"):
            lib.pfhip_op_ctc_emissions.argtypes = [_vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp]
            if hasattr(lib, "pfhip_op_ctc_greedy_plan"):
                lib.pfhip_op_ctc_greedy_plan.argtypes = [_vp, _vp, _ci, _ci, ctypes.c_longlong, _vp, _vp, _vp, _vp, _vp]
            lib.pfhip_op_ctc_align_workspace_bytes.restype = ctypes.c_size_t
            lib.pfhip_op_ctc_align_workspace_bytes.argtypes = [ctypes.c_size_t]
            lib.pfhip_op_ctc_align.argtypes = [_vp, _vp, ctypes.c_size_t, _vp, _vp, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp,
                                               ctypes.c_size_t, _vp]
        if hasattr(lib, "pfhip_op_ctc_prefix_beam"):
            lib.pfhip_op_ctc_head_topk_workspace_bytes.restype = ctypes.c_size_t
            lib.pfhip_op_ctc_head_topk_workspace_bytes.argtypes = [_ci, _ci, _ci]
            lib.pfhip_op_ctc_head_topk.argtypes = [_vp, _ci, _vp, _ci, _vp, _cf, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp,
                                                   ctypes.c_size_t, _vp]
            lib.pfhip_op_ctc_prefix_beam_workspace_bytes.restype = ctypes.c_size_t
            lib.pfhip_op_ctc_prefix_beam_workspace_bytes.argtypes = [ctypes.c_longlong, _ci, _ci, _vp]
            lib.pfhip_op_ctc_prefix_beam.argtypes = [_vp, _vp, _ci, ctypes.c_longlong, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp, _ci, _ci,
                                                     _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]
        if hasattr(lib, "pfhip_op_ctc_prefix_beam_multi"):
            lib.pfhip_op_ctc_prefix_beam_multi_workspace_bytes.restype = ctypes.c_size_t
            lib.pfhip_op_ctc_prefix_beam_multi_workspace_bytes.argtypes = [ctypes.c_longlong, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _ci]
            lib.pfhip_op_ctc_prefix_beam_multi.argtypes = [_vp, _vp, _ci, ctypes.c_longlong, _vp, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp,
                                                           _vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]
        if hasattr(lib, "pfhip_op_nbest_ctx_beam"):
            lib.pfhip_op_nbest_ctx_beam_workspace_bytes.restype = ctypes.c_size_t
            lib.pfhip_op_nbest_ctx_beam_workspace_bytes.argtypes = [ctypes.c_longlong, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _ci]
            lib.pfhip_op_nbest_ctx_beam.argtypes = [_vp, _vp, _ci, ctypes.c_longlong, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _ci,
                                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]
        if hasattr(lib, "pfhip_op_lm_score"):
            lib.pfhip_op_lm_score_workspace_bytes.restype = ctypes.c_size_t
            lib.pfhip_op_lm_score_workspace_bytes.argtypes = [_vp]
            lib.pfhip_op_lm_score.argtypes = [_vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]
            lib.pfhip_op_nbest_ctx_beam_lm_workspace_bytes.restype = ctypes.c_size_t
            lib.pfhip_op_nbest_ctx_beam_lm_workspace_bytes.argtypes = [ctypes.c_longlong, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _vp]
            lib.pfhip_op_nbest_ctx_beam_lm.argtypes = [_vp, _vp, _ci, ctypes.c_longlong, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _vp,
                                                       _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]
            lib.pfhip_op_ctc_prefix_beam_multi_lm_workspace_bytes.restype = ctypes.c_size_t
            lib.pfhip_op_ctc_prefix_beam_multi_lm_workspace_bytes.argtypes = [ctypes.c_longlong, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _vp]
            lib.pfhip_op_ctc_prefix_beam_multi_lm.argtypes = [_vp, _vp, _ci, ctypes.c_longlong, _vp, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp,
                                                              _vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]
        _bound = True
    return lib


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise PfhipError("pfhip ops need CUDA (HIP) tensors; there is no CPU path")
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ck(rc, what):
    if rc != 0:
        raise PfhipError(f"{what}: hip error {rc}")


def round_up(v, m):
    return (v + m - 1) // m * m


def best_w_scale(max_abs):
    lib = _lib()
    lib.pfhip_op_best_w_scale.restype = ctypes.c_float
    lib.pfhip_op_best_w_scale.argtypes = [ctypes.c_float]
    return float(lib.pfhip_op_best_w_scale(float(max_abs)))


def gemm_f32(A, W, bias=None, R1=None, R2=None, relu=False, M=None, N=None, guard=True, out=None, kind=0, w_scale=None):
    """C[M,N] = A[M,K] @ W[N,K]^T (+bias +R1 +R2, ReLU).  A must have ceil(M/128)*128 rows allocated
    and W ceil(N/128)*128 rows; K % 32 == 0.  w_scale: the power-of-two weight scale of the fp16 two-plane kernels
    ("auto" = best_w_scale(max |W|), what the model does per weight matrix at load; None = 1)."""
    K = A.shape[1]
    M = A.shape[0] if M is None else M
    N = W.shape[0] if N is None else N
    if out is None:
        out = torch.empty((round_up(M, 128), round_up(N, 128)), dtype=torch.float32, device=A.device)
    if w_scale is not None:
        if w_scale == "auto":
            w_scale = best_w_scale(float(W.abs().max()))
        lib = _lib()
        lib.pfhip_op_gemm_f32_scaled.argtypes = [_vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci,
                                                 ctypes.c_float, _vp]
        _ck(lib.pfhip_op_gemm_f32_scaled(_p(A), A.stride(0), _p(W), W.stride(0), _p(out), out.stride(0), _p(bias),
                                         _p(R1), R1.stride(0) if R1 is not None else 0, _p(R2),
                                         R2.stride(0) if R2 is not None else 0, M, N, K, 1 if relu else 0,
                                         1 if guard else 0, kind, float(w_scale), _stream()), "gemm")
        return out
    _ck(_lib().pfhip_op_gemm_f32_kind(_p(A), A.stride(0), _p(W), W.stride(0), _p(out), out.stride(0), _p(bias),
                                      _p(R1), R1.stride(0) if R1 is not None else 0, _p(R2),
                                      R2.stride(0) if R2 is not None else 0, M, N, K, 1 if relu else 0,
                                      1 if guard else 0, kind, _stream()), "gemm")
    return out


def set_launch_ctx(range_flag=None, exact=False):
    """The launch context of this thread's later operator calls: range_flag = an int32 device tensor of one word that the
    LayerNorm-folding kernels OR into (the caller zeroes and reads it; keep it alive until the context is reset), exact = the
    bf16 three-plane kernels.  set_launch_ctx() restores the default."""
    lib = _lib()
    lib.pfhip_op_set_launch_ctx.argtypes = [_vp, _ci]
    if range_flag is not None and (range_flag.dtype != torch.int32 or range_flag.numel() < 1):
        raise PfhipError("range_flag must be an int32 device tensor")
    _ck(lib.pfhip_op_set_launch_ctx(_p(range_flag), 1 if exact else 0), "set_launch_ctx")


def gemm_f32_ln(A, W, M=None, N=None, bias=None, R1=None, R2=None, relu=False, ln_stats=None, ln_tiles=0, ln_colsum=None, stats_out=None,
                w_scale=1.0, out=None):
    """The in-loop-split GEMM of the product path (csrc/gemm_x3.hip; gemm_x6.hip under set_launch_ctx(exact=True)) with the
    LayerNorm hand-off: ln_stats / ln_tiles / ln_colsum fold a LayerNorm of A in (W / bias from fold_layernorm), stats_out
    [rows, N / 128, 2] receives the per-tile (mean, M2) pairs of the result."""
    lib = _lib()
    K = A.shape[1]
    M = A.shape[0] if M is None else M
    N = W.shape[0] if N is None else N
    if out is None:
        out = torch.empty((round_up(M, 128), N), dtype=torch.float32, device=A.device)
    if w_scale == "auto":
        w_scale = best_w_scale(float(W.abs().max()))
    lib.pfhip_op_gemm_f32_ln.argtypes = [_vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _vp, _ci, _vp, _vp,
                                         ctypes.c_float, _vp]
    _ck(lib.pfhip_op_gemm_f32_ln(_p(A), A.stride(0), _p(W), W.stride(0), _p(out), out.stride(0), _p(bias), _p(R1),
                                 R1.stride(0) if R1 is not None else 0, _p(R2), R2.stride(0) if R2 is not None else 0, M, N, K,
                                 1 if relu else 0, _p(ln_stats), ln_tiles, _p(ln_colsum), _p(stats_out), float(w_scale), _stream()),
        "gemm_f32_ln")
    return out


def fused_ln_gemm(X, W, M, N, g=None, b=None, D=None, bias=None, R1=None, R2=None, fsmn_v=None, fsmn_w=None, relu=False, out=None,
                  eps=1e-12):
    """One streaming window: LN (if g) -> GEMM (+bias +R1 +R2 +FSMN memory of fsmn_v, ReLU) in one launch (M <= 32)."""
    K = W.shape[1]
    if out is None:
        out = torch.zeros((32, round_up(N, 128)), dtype=torch.float32, device=X.device)
    _ck(_lib().pfhip_op_fused_ln_gemm(_p(X), X.stride(0), K if D is None else D, _p(g), _p(b), eps, _p(W), W.stride(0), _p(out),
                                      out.stride(0), _p(bias), _p(R1), R1.stride(0) if R1 is not None else 0, _p(R2),
                                      R2.stride(0) if R2 is not None else 0, _p(fsmn_v), fsmn_v.stride(0) if fsmn_v is not None else 0,
                                      _p(fsmn_w), M, N, K, 1 if relu else 0, _stream()), "fused_ln_gemm")
    return out


def fold_layernorm(W, bias, g, b):
    """(W', b', colsum) for fused_gemv_1trip's algebraic LayerNorm: W' = W * g, b' = bias + W @ b, colsum = W'.sum(1) — in
    double, rounded once, as the library does at load (model_build.cpp)."""
    Wd = W.double()
    Wf = (Wd * g.double()[None, :]).float()
    bf = ((bias.double() if bias is not None else 0.0) + Wd @ b.double()).float()
    return Wf, bf, Wf.double().sum(1).float()


def fused_gemv_1trip(X, W, M, N, bias=None, ln_colsum=None, R1=None, fsmn_v=None, fsmn_w=None, relu=False, out=None, eps=1e-12):
    """One streaming window (M <= 20): (LN ->) GEMM (+bias +R1 +FSMN memory, ReLU), operands requested in one trip; with
    ln_colsum, W / bias are the folded ones of fold_layernorm."""
    K = W.shape[1]
    if out is None:
        out = torch.zeros((32, round_up(N, 128)), dtype=torch.float32, device=X.device)
    _ck(_lib().pfhip_op_fused_gemv_1trip(_p(X), X.stride(0), _p(W), W.stride(0), _p(out), out.stride(0), _p(bias), _p(ln_colsum), eps,
                                         _p(R1), R1.stride(0) if R1 is not None else 0, _p(fsmn_v),
                                         fsmn_v.stride(0) if fsmn_v is not None else 0, _p(fsmn_w), M, N, K, 1 if relu else 0, _stream()),
        "fused_gemv_1trip")
    return out


def fused_gemv_1trip_route(M, N, K, ln=False, fsmn=False):
    """What fused_gemv_1trip would launch for the shape (the launcher's own choice; nothing is launched, no device needed):
    dict(ok, ln, fs, cw, cpl, rpl, nf, waves); ok False = the shape is refused."""
    lib = _lib()
    lib.pfhip_op_fused_gemv_1trip_route.argtypes = [_ci, _ci, _ci, _ci, _ci, ctypes.POINTER(_ci)]
    out = (_ci * 8)()
    _ck(lib.pfhip_op_fused_gemv_1trip_route(int(M), int(N), int(K), 1 if ln else 0, 1 if fsmn else 0, out), "fused_gemv_1trip_route")
    ok, ln_, fs, cw, cpl, rpl, nf, waves = list(out)
    return dict(ok=bool(ok), ln=bool(ln_), fs=bool(fs), cw=cw, cpl=cpl, rpl=rpl, nf=nf, waves=waves)


def fused_ln_gemm_route(M, N, K, ln=False):
    """What fused_ln_gemm would launch for the shape: dict(kernel = "vector" | "matrix", ln, cw, mr, waves, k_blocks)."""
    lib = _lib()
    lib.pfhip_op_fused_ln_gemm_route.argtypes = [_ci, _ci, _ci, _ci, ctypes.POINTER(_ci)]
    out = (_ci * 6)()
    _ck(lib.pfhip_op_fused_ln_gemm_route(int(M), int(N), int(K), 1 if ln else 0, out), "fused_ln_gemm_route")
    kernel, ln_, cw, mr, waves, k_blocks = list(out)
    return dict(kernel={1: "vector", 2: "matrix"}.get(kernel, "none"), ln=bool(ln_), cw=cw, mr=mr, waves=waves, k_blocks=k_blocks)


def layernorm(x, g, b, D=None, Dout=None, eps=1e-12):
    M = x.shape[0]
    D = x.shape[1] if D is None else D
    Dout = D if Dout is None else Dout
    y = torch.empty((M, Dout), dtype=torch.float32, device=x.device)
    _ck(_lib().pfhip_op_layernorm(_p(x), x.stride(0), _p(y), y.stride(0), _p(g), _p(b), M, D, Dout, eps, _stream()), "layernorm")
    return y


def fsmn(v, w, off, length, res=None):
    out = torch.zeros((v.shape[0], v.shape[1]), dtype=torch.float32, device=v.device)
    B = off.numel()
    _ck(_lib().pfhip_op_fsmn(_p(v), v.stride(0), _p(w), _p(res), res.stride(0) if res is not None else 0, _p(out),
                             out.stride(0), _p(off), _p(length), B, int(length.max().item()), v.shape[1], _stream()), "fsmn")
    return out


def fsmn_shift(v, w, off, length, shift, res=None):
    """fsmn with the taps shifted into the past by `shift` frames (0, or 5 = causal: the online CT-Transformer's layers)."""
    lib = _lib()
    lib.pfhip_op_fsmn_shift.argtypes = [_vp, _ci, _vp, _vp, _ci, _vp, _ci, _vp, _vp, _ci, _ci, _ci, _ci, _vp]
    out = torch.zeros((v.shape[0], v.shape[1]), dtype=torch.float32, device=v.device)
    _ck(lib.pfhip_op_fsmn_shift(_p(v), v.stride(0), _p(w), _p(res), res.stride(0) if res is not None else 0, _p(out), out.stride(0),
                                _p(off), _p(length), off.numel(), int(length.max().item()), v.shape[1], int(shift), _stream()),
        "fsmn_shift")
    return out


def resample(x, in_off, n_in, fs_in, fs_out=16000):
    """Audio::WavResample on a packed batch (resample.hip): utterance b is x[in_off[b] : in_off[b] + n_in[b]] (float32 at fs_in).
    Returns (y, out_off, n_out): the utterances at fs_out packed back to back; offsets and counts are host int lists."""
    import numpy as np
    from . import resample_len
    n_in = [int(v) for v in n_in]
    n_out = [resample_len(fs_in, v, fs_out) for v in n_in]
    if any(v < 0 for v in n_out):
        raise PfhipError(f"unsupported rate pair {fs_in} -> {fs_out}")
    out_off = np.zeros(len(n_in), np.int64)
    out_off[1:] = np.cumsum(n_out[:-1]) if len(n_in) > 1 else out_off[1:]
    y = torch.empty(max(sum(n_out), 1), dtype=torch.float32, device=x.device)
    io = np.ascontiguousarray(in_off, np.int64)
    ni = np.ascontiguousarray(n_in, np.int32)
    _ck(_lib().pfhip_op_resample(_p(x), ctypes.c_void_p(io.ctypes.data), ctypes.c_void_p(ni.ctypes.data), len(n_in), fs_in, fs_out,
                                 _p(y), ctypes.c_void_p(out_off.ctypes.data), _stream()), "resample")
    return y, [int(v) for v in out_off], n_out


def attention(Q, K, V, q_off, q_len, kv_off, kv_len, n_head, scale, head_dim=128):
    O = torch.zeros((Q.shape[0], n_head * head_dim), dtype=torch.float32, device=Q.device)
    B = q_off.numel()
    _ck(_lib().pfhip_op_attention_hd(_p(Q), Q.stride(0), _p(K), K.stride(0), _p(V), V.stride(0), _p(O), O.stride(0),
                                     _p(q_off), _p(q_len), _p(kv_off), _p(kv_len), B, n_head, int(q_len.max().item()),
                                     scale, head_dim, _stream()), "attention")
    return O


def attention_limit(Q, K, V, q_off, q_len, kv_off, kv_len, n_head, scale, q_kv_limit, head_dim=128):
    """attention (head_dim 32, 80 or 128) with q_kv_limit: per packed query row the number of keys it may see (>= 1; int32 device)."""
    lib = _lib()
    lib.pfhip_op_attention_limit.argtypes = [_vp, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _cf, _ci, _vp, _vp]
    O = torch.zeros((Q.shape[0], n_head * head_dim), dtype=torch.float32, device=Q.device)
    _ck(lib.pfhip_op_attention_limit(_p(Q), Q.stride(0), _p(K), K.stride(0), _p(V), V.stride(0), _p(O), O.stride(0), _p(q_off), _p(q_len),
                                     _p(kv_off), _p(kv_len), q_off.numel(), n_head, int(q_len.max().item()), float(scale), int(head_dim),
                                     _p(q_kv_limit), _stream()), "attention_limit")
    return O


def attention_dk(Q, K, V, q_off, q_len, kv_off, kv_len, n_head, scale, d_k, q_kv_limit=None, out=None):
    """Attention for any head width 1 <= d_k <= 64 (the exact-width form of attention.hip's kernel), head h in columns
    [h * d_k, (h + 1) * d_k); q_kv_limit: per packed query row the number of keys it may see.  out: a [rows, >= n_head * d_k] tensor to write into (only those columns of the
    segments' rows are touched); otherwise a zero-filled [rows, n_head * d_k] one is made."""
    lib = _lib()
    O = torch.zeros((Q.shape[0], n_head * d_k), dtype=torch.float32, device=Q.device) if out is None else out
    _ck(lib.pfhip_op_attention_dk(_p(Q), Q.stride(0), _p(K), K.stride(0), _p(V), V.stride(0), _p(O), O.stride(0),
                                  _p(q_off), _p(q_len), _p(kv_off), _p(kv_len), q_off.numel(), n_head, int(q_len.max().item()),
                                  float(scale), int(d_k), _p(q_kv_limit), _stream()), "attention_dk")
    return O


def attention_fsmn_is_fused(max_len, head_dim=128):
    """Whether attention_fsmn runs as the one fused launch (only then is mem_accumulate honoured)."""
    lib = _lib()
    lib.pfhip_op_attention_fsmn_is_fused.argtypes = [_ci, _ci]
    return bool(lib.pfhip_op_attention_fsmn_is_fused(int(max_len), int(head_dim)))


def attention_fsmn(Q, K, V, off, length, n_head, scale, fsmn_w, mem, mem_accumulate=False, head_dim=128):
    """Self-attention and the SAN-M memory block of V in the encoder layer's launch: returns the context (fp32 rows); the memory goes
    into `mem` (added to it when mem_accumulate and the launch is fused)."""
    lib = _lib()
    O = torch.zeros((Q.shape[0], n_head * head_dim), dtype=torch.float32, device=Q.device)
    lib.pfhip_op_attention_fsmn.argtypes = [_vp, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _ci, _ci, _ci, _cf, _vp, _vp, _ci, _ci, _ci, _vp]
    _ck(lib.pfhip_op_attention_fsmn(_p(Q), Q.stride(0), _p(K), K.stride(0), _p(V), V.stride(0), _p(O), O.stride(0), _p(off), _p(length),
                                    off.numel(), n_head, int(length.max().item()), float(scale), _p(fsmn_w), _p(mem), mem.stride(0),
                                    1 if mem_accumulate else 0, head_dim, _stream()), "attention_fsmn")
    return O


def attention_planes(Q, K, V, q_off, q_len, kv_off, kv_len, n_head, scale):
    """attention (d_k = 128) with the context as fp16 plane images: returns (hi, lo, rows) as split_planes does."""
    lib = _lib()
    rows = round_up(Q.shape[0], 128)
    lib.pfhip_op_plane_image_bytes.restype = ctypes.c_size_t
    lib.pfhip_op_plane_image_bytes.argtypes = [_ci, _ci]
    nb = int(lib.pfhip_op_plane_image_bytes(rows, n_head * 128))
    hi = torch.zeros(nb, dtype=torch.uint8, device=Q.device)
    lo = torch.zeros(nb, dtype=torch.uint8, device=Q.device)
    lib.pfhip_op_attention_planes.argtypes = [_vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci,
                                             ctypes.c_float, _vp]
    _ck(lib.pfhip_op_attention_planes(_p(Q), Q.stride(0), _p(K), K.stride(0), _p(V), V.stride(0), _p(hi), _p(lo), rows, _p(q_off),
                                      _p(q_len), _p(kv_off), _p(kv_len), q_off.numel(), n_head, int(q_len.max().item()), Q.shape[0],
                                      float(scale), _stream()), "attention_planes")
    return hi, lo, rows


def window_attention(Q, K, V, Lq, Lk, n_head, scale, head_dim=128):
    """One streaming window: softmax(scale Q_h K_h^T) V_h for rows [0, Lq) x [0, Lk), d_k = head_dim (128 or 80)."""
    O = torch.zeros((Q.shape[0], n_head * head_dim), dtype=torch.float32, device=Q.device)
    if head_dim == 128:
        _ck(_lib().pfhip_op_window_attention(_p(Q), Q.stride(0), _p(K), K.stride(0), _p(V), V.stride(0), _p(O), O.stride(0), Lq, Lk,
                                             n_head, scale, _stream()), "window_attention")
    else:
        _ck(_lib().pfhip_op_window_attention_hd(_p(Q), Q.stride(0), _p(K), K.stride(0), _p(V), V.stride(0), _p(O), O.stride(0), Lq, Lk,
                                                n_head, scale, head_dim, _stream()), "window_attention")
    return O


def window_attention_segments(Q, K, V, q_off, q_len, kv_off, kv_len, n_head, scale, head_dim=128, fsmn_w=None, mem=None, out=None,
                              max_q_len=None, max_kv_len=None):
    """B streaming windows in one launch (segment arrays: int32 device tensors, every length <= 32), as a round of connections runs
    them.  fsmn_w / mem: also the SAN-M memory block of V into mem (self-attention).  out: a [rows, >= n_head * head_dim] tensor to
    write into (only the windows' rows and those columns are touched); otherwise a zero-filled one is made."""
    lib = _lib()
    lib.pfhip_op_window_attention_segments.argtypes = [_vp, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _cf,
                                                       _vp, _vp, _ci, _ci, _vp]
    O = torch.zeros((Q.shape[0], n_head * head_dim), dtype=torch.float32, device=Q.device) if out is None else out
    mq = int(q_len.max().item()) if max_q_len is None else max_q_len
    mk = int(kv_len.max().item()) if max_kv_len is None else max_kv_len
    _ck(lib.pfhip_op_window_attention_segments(_p(Q), Q.stride(0), _p(K), K.stride(0), _p(V), V.stride(0), _p(O), O.stride(0), _p(q_off),
                                               _p(q_len), _p(kv_off), _p(kv_len), q_off.numel(), n_head, mq, mk, float(scale), _p(fsmn_w),
                                               _p(mem), mem.stride(0) if mem is not None else 0, int(head_dim), _stream()),
        "window_attention_segments")
    return O


def fused_att_out(Q, K, V, Lq, Lk, n_head, scale, W, bias=None, R1=None, fsmn_v=None, fsmn_w=None, out=None):
    """One streaming window: attention (Lq x Lk, 4 heads of 128) and the projection of its context by W [N, 512] in one launch."""
    N = W.shape[0]
    if out is None:
        out = torch.zeros((32, N), dtype=torch.float32, device=Q.device)
    _ck(_lib().pfhip_op_fused_att_out(_p(Q), Q.stride(0), _p(K), K.stride(0), _p(V), V.stride(0), Lq, Lk, n_head, scale, _p(W), W.stride(0),
                                      _p(out), out.stride(0), _p(bias), _p(R1), R1.stride(0) if R1 is not None else 0, _p(fsmn_v),
                                      fsmn_v.stride(0) if fsmn_v is not None else 0, _p(fsmn_w), N, _stream()), "fused_att_out")
    return out


def cif(hidden, alphas, row_off, length, threshold, tail):
    B = row_off.numel()
    D = hidden.shape[1]
    stage = torch.zeros((hidden.shape[0] + B, D), dtype=torch.float32, device=hidden.device)
    n_fires = torch.zeros(B, dtype=torch.int32, device=hidden.device)
    token_num = torch.zeros(B, dtype=torch.int32, device=hidden.device)
    _ck(_lib().pfhip_op_cif(_p(hidden), hidden.stride(0), _p(alphas), _p(row_off), _p(length), B, D, threshold, tail,
                            _p(stage), _p(n_fires), _p(token_num), _stream()), "cif")
    return stage, n_fires, token_num


def cif_fires(hidden, alphas, row_off, length, threshold, tail, fire_frame=None):
    """cif by the sibling kernel that also writes fire_frame [rows + B] int32, laid out like stage's rows: fire j of utterance b at
    row_off[b] + b + j holds the scan step it happened in (0..len-1 = that row, len = the tail slot); slots past n_fires[b] keep
    what the caller put there (fire_frame given) or -1."""
    B = row_off.numel()
    D = hidden.shape[1]
    stage = torch.zeros((hidden.shape[0] + B, D), dtype=torch.float32, device=hidden.device)
    n_fires = torch.zeros(B, dtype=torch.int32, device=hidden.device)
    token_num = torch.zeros(B, dtype=torch.int32, device=hidden.device)
    if fire_frame is None:
        fire_frame = torch.full((hidden.shape[0] + B,), -1, dtype=torch.int32, device=hidden.device)
    if fire_frame.dtype != torch.int32 or fire_frame.numel() < hidden.shape[0] + B or not fire_frame.is_contiguous():
        raise PfhipError("cif_fires: fire_frame must be a contiguous int32 tensor of rows + B entries")
    _ck(_lib().pfhip_op_cif_fires(_p(hidden), hidden.stride(0), _p(alphas), _p(row_off), _p(length), B, D, threshold, tail,
                                  _p(stage), _p(n_fires), _p(token_num), _p(fire_frame), _stream()), "cif_fires")
    return stage, n_fires, token_num, fire_frame


def logsoftmax_argmax(logits, V=None, want_logp=True):
    ML = logits.shape[0]
    V = logits.shape[1] if V is None else V
    logp = torch.empty((ML, V), dtype=torch.float32, device=logits.device) if want_logp else None
    ids = torch.empty(ML, dtype=torch.int32, device=logits.device)
    _ck(_lib().pfhip_op_logsoftmax_argmax(_p(logits), logits.stride(0), ML, V, _p(logp), _p(ids), _stream()), "logsoftmax")
    return logp, ids


def logsoftmax_topk(logits, k, V=None, want_logp=True):
    """The head with the k best columns per row (csrc/topk.hip): (logp or None, ids, topk_ids [ML, k], topk_logp [ML, k]).
    Raises PfhipError (hipErrorInvalidValue = 1, nothing launched) for k outside 1..8 or V < k."""
    ML = logits.shape[0]
    V = logits.shape[1] if V is None else V
    logp = torch.empty((ML, V), dtype=torch.float32, device=logits.device) if want_logp else None
    ids = torch.empty(ML, dtype=torch.int32, device=logits.device)
    kk = max(int(k), 1)
    topk_ids = torch.empty((ML, kk), dtype=torch.int32, device=logits.device)
    topk_logp = torch.empty((ML, kk), dtype=torch.float32, device=logits.device)
    _ck(_lib().pfhip_op_logsoftmax_topk(_p(logits), logits.stride(0), ML, V, int(k), _p(logp), _p(ids), _p(topk_ids), _p(topk_logp),
                                        _stream()), "logsoftmax_topk")
    return logp, ids, topk_ids, topk_logp


def ctc_head(X, W, bias, w_scale="auto", M=None, V=None, want_lse=True):
    """The CTC head without the logits matrix (csrc/ctc_head.hip): (ids [M] int32, logp_best [M], lse [M] or None) of
    X[:M] @ W[:V]^T + bias.  w_scale as gemm_f32 ("auto" = best_w_scale(max |W|))."""
    M = X.shape[0] if M is None else M
    V = W.shape[0] if V is None else V
    K = X.shape[1]
    if w_scale == "auto":
        w_scale = best_w_scale(float(W[:V].abs().max()))
    lib = _lib()
    ids = torch.empty(M, dtype=torch.int32, device=X.device)
    logp_best = torch.empty(M, dtype=torch.float32, device=X.device)
    lse = torch.empty(M, dtype=torch.float32, device=X.device) if want_lse else None
    nbytes = int(lib.pfhip_op_ctc_head_workspace_bytes(M, V))
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=X.device)
    _ck(lib.pfhip_op_ctc_head(_p(X), X.stride(0), _p(W), W.stride(0), _p(bias), float(w_scale), M, V, K, _p(ids), _p(logp_best),
                              _p(lse), _p(ws), nbytes, _stream()), "ctc_head")
    return ids, logp_best, lse


def ctc_head_topk(X, W, bias, k, w_scale="auto", M=None, V=None, workspace_bytes=None):
    """The fused CTC head with the k best columns of every row (csrc/ctc_head.hip): (ids [M], logp_best [M], lse [M],
    topk_ids [M, k] int32, topk_logp [M, k]); the first three are ctc_head's bit for bit.  1 <= k <= 16, V >= k."""
    M = X.shape[0] if M is None else M
    V = W.shape[0] if V is None else V
    K = X.shape[1]
    if w_scale == "auto":
        w_scale = best_w_scale(float(W[:V].abs().max()))
    lib = _lib()
    dev = X.device
    ids = torch.empty(M, dtype=torch.int32, device=dev)
    logp_best = torch.empty(M, dtype=torch.float32, device=dev)
    lse = torch.empty(M, dtype=torch.float32, device=dev)
    kk = max(int(k), 1)
    topk_ids = torch.full((M, kk), -7, dtype=torch.int32, device=dev)
    topk_logp = torch.full((M, kk), float("nan"), dtype=torch.float32, device=dev)
    nbytes = int(lib.pfhip_op_ctc_head_topk_workspace_bytes(M, V, int(k))) if workspace_bytes is None else int(workspace_bytes)
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=dev)
    _ck(lib.pfhip_op_ctc_head_topk(_p(X), X.stride(0), _p(W), W.stride(0), _p(bias), float(w_scale), M, V, K, int(k), _p(ids),
                                   _p(logp_best), _p(lse), _p(topk_ids), _p(topk_logp), _p(ws), nbytes, _stream()), "ctc_head_topk")
    return ids, logp_best, lse, topk_ids, topk_logp


def ctc_prefix_beam(topk_ids, topk_logp, row_off, length, vocab, first_beam, second_beam, nbest=None, max_tokens=None, blank=0,
                    graph=None, workspace_bytes=None, rows=None):
    """CTC prefix beam search with hotwords (csrc/ctc_beam.hip; include/pfhip_ops.h states the recurrence and the tie rule) over
    topk_ids / topk_logp [rows, k]; row_off / length: int32 device tensors [B]; graph: a ContextGraph or None.  Returns
    (n_hyp [B], ids [B, nbest, max_tokens], n_tokens [B, nbest], score, ctc_score, ctx_score [B, nbest]).  rows: the row count the
    kernel is told (default: all of the tensors'; fewer leaves the rest as padding, and the workspace is sized for all)."""
    lib = _lib()
    all_rows, k = int(topk_ids.shape[0]), int(topk_ids.shape[1])
    rows = all_rows if rows is None else min(int(rows), all_rows)
    B = int(row_off.numel())
    nbest = int(second_beam) if nbest is None else int(nbest)
    max_tokens = rows if max_tokens is None else int(max_tokens)
    dev = topk_ids.device
    nb = max(nbest, 1)
    n_hyp = torch.full((max(B, 1),), -7, dtype=torch.int32, device=dev)
    ids = torch.full((max(B, 1), nb, max(max_tokens, 1)), -7, dtype=torch.int32, device=dev)
    n_tokens = torch.full((max(B, 1), nb), -7, dtype=torch.int32, device=dev)
    score, ctc_score, ctx_score = (torch.full((max(B, 1), nb), float("nan"), dtype=torch.float32, device=dev) for _ in range(3))
    gh = graph.handle if graph is not None else None
    nbytes = int(lib.pfhip_op_ctc_prefix_beam_workspace_bytes(all_rows, B, int(second_beam), gh)) if workspace_bytes is None else int(workspace_bytes)
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.int32, device=dev)
    if max_tokens != ids.shape[2]:                                   # max_tokens 0: the kernel gets a stride of 0 and no buffer use
        ids = ids[:, :, :0]
    _ck(lib.pfhip_op_ctc_prefix_beam(_p(topk_ids), _p(topk_logp), k, rows, _p(row_off), _p(length), B, int(vocab), int(blank),
                                     int(first_beam), int(second_beam), gh, nbest, max_tokens, _p(n_hyp), _p(ids) if max_tokens else None,
                                     _p(n_tokens), _p(score), _p(ctc_score), _p(ctx_score), _p(ws), nbytes, _stream()), "ctc_prefix_beam")
    return n_hyp[:B], ids[:B], n_tokens[:B], score[:B], ctc_score[:B], ctx_score[:B]


def ctc_prefix_beam_multi(topk_ids, topk_logp, row_off, length, vocab, first_beam, second_beam, nbest, graph_of=None, graphs=(),
                          max_tokens=None, blank=0, workspace_bytes=None, rows=None, out=None):
    """ctc_prefix_beam with every utterance on its own parameters, in one launch (pfhip_op_ctc_prefix_beam_multi): first_beam,
    second_beam, nbest and graph_of are host sequences [B] (first_beam 0: no search for that utterance; graph_of -1: no graph),
    graphs a sequence of ContextGraph.  Utterance b reads the first first_beam[b] columns of its rows.  Returns ctc_prefix_beam's
    tuple with nbest_max = the largest nbest among the searching utterances as the hypothesis stride.  out: that tuple to write
    into instead of fresh tensors (a refusal must leave it as it was)."""
    lib = _lib()
    all_rows, k = int(topk_ids.shape[0]), int(topk_ids.shape[1])
    rows = all_rows if rows is None else min(int(rows), all_rows)
    B = int(row_off.numel())
    arr = lambda v: (ctypes.c_int * max(B, 1))(*[int(x) for x in v])
    graph_of = [-1] * B if graph_of is None else graph_of
    if not (len(first_beam) == len(second_beam) == len(nbest) == len(graph_of) == B):
        raise PfhipError("ctc_prefix_beam_multi: one first_beam, second_beam, nbest and graph_of per utterance")
    fb, sb, nb, go = arr(first_beam), arr(second_beam), arr(nbest), arr(graph_of)
    handles = (ctypes.c_void_p * max(len(graphs), 1))(*[g.handle for g in graphs])
    nb_max = max([int(n) for f, n in zip(first_beam, nbest) if int(f) > 0] + [1])
    max_tokens = rows if max_tokens is None else int(max_tokens)
    dev = topk_ids.device
    if out is None:
        n_hyp = torch.full((max(B, 1),), -7, dtype=torch.int32, device=dev)
        ids = torch.full((max(B, 1), nb_max, max(max_tokens, 1)), -7, dtype=torch.int32, device=dev)
        n_tokens = torch.full((max(B, 1), nb_max), -7, dtype=torch.int32, device=dev)
        score, ctc_score, ctx_score = (torch.full((max(B, 1), nb_max), float("nan"), dtype=torch.float32, device=dev) for _ in range(3))
    else:
        n_hyp, ids, n_tokens, score, ctc_score, ctx_score = out
    if workspace_bytes is None:
        nbytes = int(lib.pfhip_op_ctc_prefix_beam_multi_workspace_bytes(all_rows, B, k, fb, sb, nb, go, handles, len(graphs)))
    else:
        nbytes = int(workspace_bytes)
    ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.int32, device=dev)
    if max_tokens != ids.shape[2]:
        ids = ids[:, :, :0]
    _ck(lib.pfhip_op_ctc_prefix_beam_multi(_p(topk_ids), _p(topk_logp), k, rows, _p(row_off), _p(length), B, int(vocab), int(blank), fb, sb, nb,
                                           go, handles, len(graphs), max_tokens, _p(n_hyp), _p(ids) if max_tokens else None, _p(n_tokens),
                                           _p(score), _p(ctc_score), _p(ctx_score), _p(ws), nbytes, _stream()), "ctc_prefix_beam_multi")
    return n_hyp[:B], ids[:B], n_tokens[:B], score[:B], ctc_score[:B], ctx_score[:B]


def nbest_ctx_beam(cand_ids, cand_logp, row_off, length, vocab, width, beam, nbest, graph_of=None, graphs=(), max_tokens=None,
                   workspace_bytes=None, rows=None, out=None):
    """Hotword-biased beam search over a non-autoregressive head's candidates (csrc/nar_beam.hip; include/pfhip_ops.h states the
    recurrence and the tie rule): cand_ids / cand_logp [rows, k <= 8] device tensors, row_off / length int32 device tensors [B];
    width, beam, nbest and graph_of host sequences [B] (graph_of -1: no graph), graphs a sequence of ContextGraph.  Utterance b
    reads the first width[b] columns of its rows and gives one token per row.  Returns (n_hyp [B], ids [B, nbest_max, max_tokens],
    n_tokens [B, nbest_max], score, am_score, ctx_score [B, nbest_max]).  rows: the row count the kernel is told (default: all of the
    tensors'; the workspace is sized for all).  out: that tuple to write into (a refusal must leave it as it was)."""
    lib = _lib()
    if not hasattr(lib, "pfhip_op_nbest_ctx_beam"):
        raise PfhipError("nbest_ctx_beam: this libpfhip has no pfhip_op_nbest_ctx_beam")
    all_rows, k = int(cand_ids.shape[0]), int(cand_ids.shape[1])
    rows = all_rows if rows is None else min(int(rows), all_rows)
    B = int(row_off.numel())
    arr = lambda v: (ctypes.c_int * max(B, 1))(*[int(x) for x in v])
    graph_of = [-1] * B if graph_of is None else graph_of
    if not (len(width) == len(beam) == len(nbest) == len(graph_of) == B):
        raise PfhipError("nbest_ctx_beam: one width, beam, nbest and graph_of per utterance")
    wd, bm, nb, go = arr(width), arr(beam), arr(nbest), arr(graph_of)
    handles = (ctypes.c_void_p * max(len(graphs), 1))(*[g.handle for g in graphs])
    nb_max = max([int(n) for n in nbest] + [1])
    max_tokens = rows if max_tokens is None else int(max_tokens)
    dev = cand_ids.device
    if out is None:
        n_hyp = torch.full((max(B, 1),), -7, dtype=torch.int32, device=dev)
        ids = torch.full((max(B, 1), nb_max, max(max_tokens, 1)), -7, dtype=torch.int32, device=dev)
        n_tokens = torch.full((max(B, 1), nb_max), -7, dtype=torch.int32, device=dev)
        score, am_score, ctx_score = (torch.full((max(B, 1), nb_max), float("nan"), dtype=torch.float32, device=dev) for _ in range(3))
    else:
        n_hyp, ids, n_tokens, score, am_score, ctx_score = out
        if tuple(ids.shape) != (max(B, 1), nb_max, max(max_tokens, 1)) or any(tuple(t.shape) != (max(B, 1), nb_max)
                                                                                for t in (n_tokens, score, am_score, ctx_score)):
            raise PfhipError("nbest_ctx_beam: out must be shaped [B, nbest_max, max(max_tokens, 1)] and [B, nbest_max]")
    if workspace_bytes is None:
        nbytes = int(lib.pfhip_op_nbest_ctx_beam_workspace_bytes(all_rows, B, k, wd, bm, nb, go, handles, len(graphs)))
    else:
        nbytes = int(workspace_bytes)
    ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.int32, device=dev)
    if max_tokens == 0:                                              # the kernel gets a stride of 0 and no buffer
        ids = ids[:, :, :0]
    _ck(lib.pfhip_op_nbest_ctx_beam(_p(cand_ids), _p(cand_logp), k, rows, _p(row_off), _p(length), B, int(vocab), wd, bm, nb, go, handles,
                                    len(graphs), max_tokens, _p(n_hyp), _p(ids) if max_tokens else None, _p(n_tokens), _p(score),
                                    _p(am_score), _p(ctx_score), _p(ws), nbytes, _stream()), "nbest_ctx_beam")
    return n_hyp[:B], ids[:B], n_tokens[:B], score[:B], am_score[:B], ctx_score[:B]


def ctc_prefix_beam_multi_lm(topk_ids, topk_logp, row_off, length, vocab, first_beam, second_beam, nbest, lm, graph_of=None, graphs=(),
                             max_tokens=None, blank=0, workspace_bytes=None, rows=None):
    """ctc_prefix_beam_multi with a token n-gram language model fused in (pfhip_op_ctc_prefix_beam_multi_lm): lm an LmGraph, or None
    for the sibling's launch.  Returns ctc_prefix_beam_multi's tuple and lm_score [B, nbest_max] behind it; score includes lm_score."""
    lib = _lib()
    if not hasattr(lib, "pfhip_op_ctc_prefix_beam_multi_lm"):
        raise PfhipError("ctc_prefix_beam_multi_lm: this libpfhip has no pfhip_op_ctc_prefix_beam_multi_lm")
    all_rows, k = int(topk_ids.shape[0]), int(topk_ids.shape[1])
    rows = all_rows if rows is None else min(int(rows), all_rows)
    B = int(row_off.numel())
    arr = lambda v: (ctypes.c_int * max(B, 1))(*[int(x) for x in v])
    graph_of = [-1] * B if graph_of is None else graph_of
    if not (len(first_beam) == len(second_beam) == len(nbest) == len(graph_of) == B):
        raise PfhipError("ctc_prefix_beam_multi_lm: one first_beam, second_beam, nbest and graph_of per utterance")
    fb, sb, nb, go = arr(first_beam), arr(second_beam), arr(nbest), arr(graph_of)
    handles = (ctypes.c_void_p * max(len(graphs), 1))(*[g.handle for g in graphs])
    lmh = lm.handle if lm is not None else None
    nb_max = max([int(n) for f, n in zip(first_beam, nbest) if int(f) > 0] + [1])
    max_tokens = rows if max_tokens is None else int(max_tokens)
    dev = topk_ids.device
    n_hyp = torch.full((max(B, 1),), -7, dtype=torch.int32, device=dev)
    ids = torch.full((max(B, 1), nb_max, max(max_tokens, 1)), -7, dtype=torch.int32, device=dev)
    n_tokens = torch.full((max(B, 1), nb_max), -7, dtype=torch.int32, device=dev)
    score, ctc_score, ctx_score, lm_score = (torch.full((max(B, 1), nb_max), float("nan"), dtype=torch.float32, device=dev) for _ in range(4))
    if workspace_bytes is None:
        nbytes = int(lib.pfhip_op_ctc_prefix_beam_multi_lm_workspace_bytes(all_rows, B, k, fb, sb, nb, go, handles, len(graphs), lmh))
    else:
        nbytes = int(workspace_bytes)
    ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.int32, device=dev)
    if max_tokens != ids.shape[2]:
        ids = ids[:, :, :0]
    _ck(lib.pfhip_op_ctc_prefix_beam_multi_lm(_p(topk_ids), _p(topk_logp), k, rows, _p(row_off), _p(length), B, int(vocab), int(blank), fb, sb,
                                              nb, go, handles, len(graphs), lmh, max_tokens, _p(n_hyp), _p(ids) if max_tokens else None,
                                              _p(n_tokens), _p(score), _p(ctc_score), _p(ctx_score), _p(lm_score), _p(ws), nbytes, _stream()),
        "ctc_prefix_beam_multi_lm")
    return n_hyp[:B], ids[:B], n_tokens[:B], score[:B], ctc_score[:B], ctx_score[:B], lm_score[:B]


def nbest_ctx_beam_lm(cand_ids, cand_logp, row_off, length, vocab, width, beam, nbest, lm, graph_of=None, graphs=(), max_tokens=None,
                      workspace_bytes=None, rows=None):
    """nbest_ctx_beam with a token n-gram language model fused in (pfhip_op_nbest_ctx_beam_lm): lm an LmGraph, or None for the
    sibling's launch.  Returns nbest_ctx_beam's tuple and lm_score [B, nbest_max] behind it; score includes lm_score."""
    lib = _lib()
    if not hasattr(lib, "pfhip_op_nbest_ctx_beam_lm"):
        raise PfhipError("nbest_ctx_beam_lm: this libpfhip has no pfhip_op_nbest_ctx_beam_lm")
    all_rows, k = int(cand_ids.shape[0]), int(cand_ids.shape[1])
    rows = all_rows if rows is None else min(int(rows), all_rows)
    B = int(row_off.numel())
    arr = lambda v: (ctypes.c_int * max(B, 1))(*[int(x) for x in v])
    graph_of = [-1] * B if graph_of is None else graph_of
    if not (len(width) == len(beam) == len(nbest) == len(graph_of) == B):
        raise PfhipError("nbest_ctx_beam_lm: one width, beam, nbest and graph_of per utterance")
    wd, bm, nb, go = arr(width), arr(beam), arr(nbest), arr(graph_of)
    handles = (ctypes.c_void_p * max(len(graphs), 1))(*[g.handle for g in graphs])
    lmh = lm.handle if lm is not None else None
    nb_max = max([int(n) for n in nbest] + [1])
    max_tokens = rows if max_tokens is None else int(max_tokens)
    dev = cand_ids.device
    n_hyp = torch.full((max(B, 1),), -7, dtype=torch.int32, device=dev)
    ids = torch.full((max(B, 1), nb_max, max(max_tokens, 1)), -7, dtype=torch.int32, device=dev)
    n_tokens = torch.full((max(B, 1), nb_max), -7, dtype=torch.int32, device=dev)
    score, am_score, ctx_score, lm_score = (torch.full((max(B, 1), nb_max), float("nan"), dtype=torch.float32, device=dev) for _ in range(4))
    if workspace_bytes is None:
        nbytes = int(lib.pfhip_op_nbest_ctx_beam_lm_workspace_bytes(all_rows, B, k, wd, bm, nb, go, handles, len(graphs), lmh))
    else:
        nbytes = int(workspace_bytes)
    ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.int32, device=dev)
    if max_tokens == 0:                                              # the kernel gets a stride of 0 and no buffer
        ids = ids[:, :, :0]
    _ck(lib.pfhip_op_nbest_ctx_beam_lm(_p(cand_ids), _p(cand_logp), k, rows, _p(row_off), _p(length), B, int(vocab), wd, bm, nb, go, handles,
                                       len(graphs), lmh, max_tokens, _p(n_hyp), _p(ids) if max_tokens else None, _p(n_tokens), _p(score),
                                       _p(am_score), _p(ctx_score), _p(lm_score), _p(ws), nbytes, _stream()), "nbest_ctx_beam_lm")
    return n_hyp[:B], ids[:B], n_tokens[:B], score[:B], am_score[:B], ctx_score[:B], lm_score[:B]


def lm_score(ids, length, lm):
    """Sentences scored by a token n-gram language model (csrc/lm_score.hip; pfhip_op_lm_score in include/pfhip_ops.h): ids int32
    [B, max_len] and length int32 [B] device tensors, lm an LmGraph.  Returns (tok_w [B, max_len], eos_w [B], total [B])."""
    lib = _lib()
    if not hasattr(lib, "pfhip_op_lm_score"):
        raise PfhipError("lm_score: this libpfhip has no pfhip_op_lm_score")
    B, max_len = int(ids.shape[0]), int(ids.shape[1])
    dev = ids.device
    tok_w = torch.full((max(B, 1), max(max_len, 1)), float("nan"), dtype=torch.float32, device=dev)[:, :max_len].contiguous()
    eos_w, total = (torch.full((max(B, 1),), float("nan"), dtype=torch.float32, device=dev) for _ in range(2))
    nbytes = int(lib.pfhip_op_lm_score_workspace_bytes(lm.handle))
    ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.int32, device=dev)
    _ck(lib.pfhip_op_lm_score(_p(ids) if max_len else None, _p(length), B, max_len, lm.handle, _p(tok_w) if max_len else None, _p(eos_w),
                              _p(total), _p(ws), nbytes, _stream()), "lm_score")
    return tok_w[:B], eos_w[:B], total[:B]


def ctc_collapse_chunk():
    return int(_lib().pfhip_op_ctc_collapse_chunk())


def ctc_collapse(frame_ids, frame_logp, row_off, length, max_tokens, blank=0, fill=-1):
    """CTC collapse per utterance (csrc/ctc_head.hip): (ids, tok_frame, tok_logp [B, max_tokens], token_num [B]).  Slots past
    token_num[b] keep `fill` (NaN for tok_logp)."""
    B = row_off.numel()
    dev = frame_ids.device
    ids = torch.full((B, max_tokens), fill, dtype=torch.int32, device=dev)
    tok_frame = torch.full((B, max_tokens), fill, dtype=torch.int32, device=dev)
    tok_logp = torch.full((B, max_tokens), float("nan"), dtype=torch.float32, device=dev)
    token_num = torch.full((B,), fill, dtype=torch.int32, device=dev)
    _ck(_lib().pfhip_op_ctc_collapse(_p(frame_ids), _p(frame_logp), _p(row_off), _p(length), B, int(blank), int(max_tokens), _p(ids),
                                     _p(tok_frame), _p(tok_logp), _p(token_num), _stream()), "ctc_collapse")
    return ids, tok_frame, tok_logp, token_num


class CtcLabels:
    """The labels of a batch as the alignment kernels take them: per-utterance label lists and frame counts on the host, and their
    device arrays (labels packed, lab_off, n_lab, len int32; e_off int64 = the prefix sums of len * (n_lab + 1))."""

    def __init__(self, labels, length, device="cuda"):
        self.lists = [[int(x) for x in y] for y in labels]
        self.length = [int(n) for n in length]
        assert len(self.lists) == len(self.length)
        self.B = len(self.lists)
        self.n = [len(y) for y in self.lists]
        self.lab_off_h = [sum(self.n[:b]) for b in range(self.B)]
        sizes = [self.length[b] * (self.n[b] + 1) for b in range(self.B)]
        self.e_off_h = [sum(sizes[:b]) for b in range(self.B)]
        self.e_floats = sum(sizes)
        i32 = lambda v: torch.tensor(list(v) or [0], dtype=torch.int32, device=device)
        self.labels = i32([x for y in self.lists for x in y])
        self.lab_off, self.n_lab, self.len = i32(self.lab_off_h), i32(self.n), i32(self.length)
        self.e_off = torch.tensor(self.e_off_h or [0], dtype=torch.int64, device=device)

    def cut(self, E, b):
        """E_b [len, n_lab + 1] of a packed E (a host array or a tensor)."""
        o, N, C = self.e_off_h[b], self.length[b], self.n[b] + 1
        return E[o:o + N * C].reshape(N, C)


def ctc_emissions(X, W, bias, lse, row_off, lab, blank=0, V=None, E=None, e_base=0):
    """The emissions of the labels asked for (csrc/ctc_align.hip): packed E (float32, lab.e_floats) of X rows row_off[b] .. + lab.len[b]
    against W rows blank | lab.lists[b], minus lse per row.  row_off: a device int32 tensor.  E / e_base: write into a caller's buffer
    e_base floats in (tests put sentinels around it)."""
    V = W.shape[0] if V is None else V
    if E is None:
        E = torch.empty(max(lab.e_floats, 1), dtype=torch.float32, device=X.device)
    e_off = lab.e_off + int(e_base)
    _ck(_lib().pfhip_op_ctc_emissions(_p(X), X.stride(0), _p(W), W.stride(0), _p(bias), _p(lse), _p(row_off), _p(lab.len), _p(lab.lab_off),
                                      _p(lab.n_lab), _p(lab.labels), _p(e_off), lab.B, X.shape[1], V, int(blank), _p(E), _stream()),
        "ctc_emissions")
    return E


def ctc_greedy_plan(token_num, speech_len, maxT, cap_floats):
    """The sizes of a greedy alignment from the collapse's counts, on the device (csrc/ctc_align.hip ctc_greedy_plan_kernel):
    (n_lab, lab_off [B] int32, e_off [B] int64, total: int64 scalar tensor).  token_num / speech_len: device int32 tensors."""
    B = token_num.numel()
    dev = token_num.device
    n_lab = torch.full((max(B, 1),), -77, dtype=torch.int32, device=dev)
    lab_off = torch.full((max(B, 1),), -77, dtype=torch.int32, device=dev)
    e_off = torch.full((max(B, 1),), -77, dtype=torch.int64, device=dev)
    total = torch.full((1,), -77, dtype=torch.int64, device=dev)
    _ck(_lib().pfhip_op_ctc_greedy_plan(_p(token_num), _p(speech_len), B, int(maxT), int(cap_floats), _p(n_lab), _p(lab_off), _p(e_off),
                                        _p(total), _stream()), "ctc_greedy_plan")
    return n_lab[:B], lab_off[:B], e_off[:B], total[0]


def ctc_align_workspace_bytes(e_floats):
    return int(_lib().pfhip_op_ctc_align_workspace_bytes(int(e_floats)))


def ctc_align(E, lab, max_tokens=None, want_logp=True, workspace_bytes=None):
    """Viterbi over the CTC trellis and the token spans (csrc/ctc_align.hip; include/pfhip_ops.h states the recurrence):
    (tok_begin, tok_end [B, max_tokens] int32, tok_logp [B, max_tokens] or None, score [B]).  An n_lab above max_tokens is refused here,
    before the launch (PfhipError), as the labels are the host's."""
    lib = _lib()
    max_tokens = max(lab.n + [0]) if max_tokens is None else int(max_tokens)
    if any(n > max_tokens for n in lab.n):
        raise PfhipError("ctc_align: an utterance has more labels than max_tokens")
    dev = lab.len.device
    tok_begin = torch.full((lab.B, max(max_tokens, 1)), -7, dtype=torch.int32, device=dev)
    tok_end = torch.full((lab.B, max(max_tokens, 1)), -7, dtype=torch.int32, device=dev)
    tok_logp = torch.full((lab.B, max(max_tokens, 1)), float("nan"), dtype=torch.float32, device=dev) if want_logp else None
    score = torch.full((max(lab.B, 1),), float("nan"), dtype=torch.float32, device=dev)
    nbytes = ctc_align_workspace_bytes(lab.e_floats) if workspace_bytes is None else int(workspace_bytes)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _ck(lib.pfhip_op_ctc_align(_p(E), _p(lab.e_off), lab.e_floats, _p(lab.len), _p(lab.n_lab), _p(lab.labels), _p(lab.lab_off), lab.B,
                               max_tokens, _p(tok_begin), _p(tok_end), _p(tok_logp), _p(score), _p(ws), nbytes, _stream()), "ctc_align")
    return tok_begin[:, :max_tokens], tok_end[:, :max_tokens], None if tok_logp is None else tok_logp[:, :max_tokens], score[:lab.B]


# ---- pre-split operands (csrc/gemm_p3.hip) ------------------------------------------------------------------------------------
def split_planes(X, rows=None, scale=1.0, rows_valid=None):
    """fp32 [R, K] (device) -> (hi, lo) plane images (uint8 tensors of plane_image_bytes each), rows padded to a multiple of 128."""
    lib = _lib()
    R, K = X.shape
    rows_valid = R if rows_valid is None else rows_valid
    rows = round_up(R if rows is None else rows, 128)
    lib.pfhip_op_plane_image_bytes.restype = ctypes.c_size_t
    lib.pfhip_op_plane_image_bytes.argtypes = [_ci, _ci]
    nb = int(lib.pfhip_op_plane_image_bytes(rows, K))
    hi = torch.empty(nb, dtype=torch.uint8, device=X.device)
    lo = torch.empty(nb, dtype=torch.uint8, device=X.device)
    lib.pfhip_op_split_planes.argtypes = [_vp, _ci, _ci, _ci, _ci, ctypes.c_float, _vp, _vp, _vp]
    _ck(lib.pfhip_op_split_planes(_p(X), X.stride(0), rows_valid, rows, K, float(scale), _p(hi), _p(lo), _stream()), "split_planes")
    return hi, lo, rows


def planes_to_float(hi, lo, rows, K):
    """Inverse of the image layout (host side, for tests): -> float64 [rows, K] = hi + lo."""
    import numpy as np
    out = np.zeros((rows, K), np.float64)
    for img in (hi, lo):
        a = img.cpu().numpy().view(np.float16).reshape(K // 16, rows, 2, 8).astype(np.float64)
        swap = ((np.arange(rows) >> 3) & 1).astype(bool)
        a[:, swap] = a[:, swap][:, :, ::-1]
        out += a.transpose(1, 0, 2, 3).reshape(rows, K)
    return out


def gemm_p3(A_img, W_img, M, N, K, w_scale=1.0, bias=None, R1=None, relu=False, want_c=True, want_planes=False, ln_stats=None,
            ln_tiles=0, ln_colsum=None, stats_out=None, out=None, out_planes=None, tile_rows=0, tile_cols=0):
    """A_img / W_img: (hi, lo, rows) from split_planes.  Returns (C or None, (hi, lo, rows) of C or None).  out / out_planes: reuse
    buffers of an earlier call (timing loops).  tile_cols=256 forces the 256 x 256 tile (RuntimeError for a form it does not serve)."""
    lib = _lib()
    ah, al, ra = A_img
    wh, wl, rw = W_img
    Mp = round_up(M, 128)
    C = (out if out is not None else torch.empty((Mp, N), dtype=torch.float32, device=ah.device)) if want_c else None
    P = None
    if want_planes and out_planes is not None:
        P = out_planes
    elif want_planes:
        nb = int(lib.pfhip_op_plane_image_bytes(Mp, N))
        P = (torch.zeros(nb, dtype=torch.uint8, device=ah.device), torch.zeros(nb, dtype=torch.uint8, device=ah.device), Mp)
    lib.pfhip_op_gemm_p3.argtypes = [_vp, _vp, _ci, _vp, _vp, _ci, ctypes.c_float, _vp, _ci, _vp, _vp, _ci, _vp, _vp, _ci, _ci, _ci, _ci, _ci,
                                     _vp, _ci, _vp, _vp, _ci, _vp]
    args = (_p(ah), _p(al), ra, _p(wh), _p(wl), rw, float(w_scale), _p(C), N if want_c else 0, _p(P[0]) if P else None,
            _p(P[1]) if P else None, Mp, _p(bias), _p(R1), R1.stride(0) if R1 is not None else 0, M, N, K,
            1 if relu else 0, _p(ln_stats), ln_tiles, _p(ln_colsum), _p(stats_out), tile_rows)
    if tile_cols:
        lib.pfhip_op_gemm_p3_cols.argtypes = lib.pfhip_op_gemm_p3.argtypes[:-1] + [_ci, _vp]
        _ck(lib.pfhip_op_gemm_p3_cols(*args, tile_cols, _stream()), "gemm_p3")
    else:
        _ck(lib.pfhip_op_gemm_p3(*args, _stream()), "gemm_p3")
    return C, P


def gemm_p3_wide_launches():
    """Launches of this process that the 256 x 256 tile of gemm_p3 has served."""
    lib = _lib()
    lib.pfhip_op_gemm_p3_wide_launches.restype = ctypes.c_long
    return int(lib.pfhip_op_gemm_p3_wide_launches())


# ---- K | V as row-major planes (csrc/attention_p3.hip) ------------------------------------------------------------------------------
def split_rows(X, ldp=None, out=None, col=0):
    """fp32 [R, C] (device) -> row-major planes (hi, lo): float16 tensors [R, ldp], X in columns col .. col + C - 1."""
    lib = _lib()
    R, C = X.shape
    ldp = C if ldp is None else ldp
    if out is None:
        out = (torch.zeros((R, ldp), dtype=torch.float16, device=X.device), torch.zeros((R, ldp), dtype=torch.float16, device=X.device))
    hi, lo = out
    lib.pfhip_op_split_rows.argtypes = [_vp, _ci, _ci, _ci, _vp, _vp, _ci, _vp]
    _ck(lib.pfhip_op_split_rows(_p(X), X.stride(0), R, C, hi.data_ptr() + 2 * col, lo.data_ptr() + 2 * col, ldp, _stream()), "split_rows")
    return hi, lo


def gemm_p3_qkv(A_img, W_img, M, N, K, q_cols, w_scale=1.0, bias=None, ln_stats=None, ln_tiles=0, ln_colsum=None, tile_rows=0):
    """The QKV projection on plane-image operands: returns (C [Mp, q_cols] fp32, (kv_hi, kv_lo) float16 [Mp, N - q_cols])."""
    lib = _lib()
    ah, al, ra = A_img
    wh, wl, rw = W_img
    Mp = round_up(M, 128)
    C = torch.zeros((Mp, q_cols), dtype=torch.float32, device=ah.device)
    kvh = torch.zeros((Mp, N - q_cols), dtype=torch.float16, device=ah.device)
    kvl = torch.zeros((Mp, N - q_cols), dtype=torch.float16, device=ah.device)
    lib.pfhip_op_gemm_p3_qkv.argtypes = [_vp, _vp, _ci, _vp, _vp, _ci, ctypes.c_float, _vp, _ci, _vp, _vp, _ci, _ci, _vp, _ci, _ci, _ci, _vp, _ci,
                                         _vp, _ci, _vp]
    _ck(lib.pfhip_op_gemm_p3_qkv(_p(ah), _p(al), ra, _p(wh), _p(wl), rw, float(w_scale), _p(C), q_cols, _p(kvh), _p(kvl), N - q_cols, q_cols,
                                 _p(bias), M, N, K, _p(ln_stats), ln_tiles, _p(ln_colsum), tile_rows, _stream()), "gemm_p3_qkv")
    return C, (kvh, kvl)


def attention_kvplanes(Q, kv, v_col, q_off, q_len, kv_off, kv_len, n_head, scale, fsmn_w=None, mem=None, mem_accumulate=False,
                       want_planes=False):
    """attention (d_k = 128) on K | V given as row-major planes kv = (hi, lo) float16 [R, ld] (K at column 0, V at column v_col).
    Returns the context as fp32 rows, or as (hi, lo, rows) plane images with want_planes."""
    lib = _lib()
    kvh, kvl = kv
    O, P = None, None
    rows = round_up(Q.shape[0], 128)
    if want_planes:
        lib.pfhip_op_plane_image_bytes.restype = ctypes.c_size_t
        lib.pfhip_op_plane_image_bytes.argtypes = [_ci, _ci]
        nb = int(lib.pfhip_op_plane_image_bytes(rows, n_head * 128))
        P = (torch.zeros(nb, dtype=torch.uint8, device=Q.device), torch.zeros(nb, dtype=torch.uint8, device=Q.device), rows)
    else:
        O = torch.zeros((Q.shape[0], n_head * 128), dtype=torch.float32, device=Q.device)
    lib.pfhip_op_attention_kvplanes.argtypes = [_vp, _ci, _vp, _vp, _ci, _ci, _ci, _vp, _ci, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci,
                                                ctypes.c_float, _vp, _vp, _ci, _ci, _vp]
    _ck(lib.pfhip_op_attention_kvplanes(_p(Q), Q.stride(0), _p(kvh), _p(kvl), kvh.stride(0), v_col, kvh.shape[0], _p(O),
                                        O.stride(0) if O is not None else 0, _p(P[0]) if P else None, _p(P[1]) if P else None, rows,
                                        _p(q_off), _p(q_len), _p(kv_off), _p(kv_len), q_off.numel(), n_head, int(q_len.max().item()),
                                        Q.shape[0], float(scale), _p(fsmn_w), _p(mem), mem.stride(0) if mem is not None else 0,
                                        1 if mem_accumulate else 0, _stream()), "attention_kvplanes")
    return P if want_planes else O


# ---- the scan, cache and row kernels (csrc/stream.hip, vad.hip, rowops.hip, blstm.hip) ------------------------------------------------
def _hi(values):
    """A host int32 array for an entry that takes per-connection HOST arrays: (keep-alive array, pointer)."""
    import numpy as np
    a = np.ascontiguousarray(values, np.int32)
    return a, ctypes.c_void_p(a.ctypes.data)


_ll = ctypes.c_longlong


def cif_stream(enc, alphas, row_off, n, is_last, pre, suf, carry, D, threshold, tail, emb, n_fire):
    """CifSearch for B connections in one launch.  row_off / n / is_last / pre / suf: host int sequences; carry [B, >= D + 1]
    (hidden, then the integrate scalar; replaced in place); emb [B, emb_rows, D] and n_fire [B] int32 are written."""
    B = len(n)
    lib = _lib()
    lib.pfhip_op_cif_stream.argtypes = [_vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _ci, _ci, _cf, _cf, _vp, _ci, _vp, _vp]
    ro, n_, il, pr, su = _hi(row_off), _hi(n), _hi(is_last), _hi(pre), _hi(suf)
    _ck(lib.pfhip_op_cif_stream(_p(enc), enc.stride(0), _p(alphas), ro[1], n_[1], il[1], pr[1], su[1], _p(carry), carry.stride(0), B, D,
                                float(threshold), float(tail), _p(emb), emb.shape[1], _p(n_fire), _stream()), "cif_stream")


def cif_stream_fires(enc, alphas, row_off, n, is_last, pre, suf, carry, D, threshold, tail, emb, n_fire, fire_step):
    """cif_stream by the sibling kernel that also writes fire_step [B, emb_rows] int32: the scan step in which each stored token
    fired (0 = the carry slot, 1..n = window rows 0..n-1, n + 1 = the tail slot).  Slots past the stored fires are left alone."""
    B = len(n)
    lib = _lib()
    lib.pfhip_op_cif_stream_fires.argtypes = [_vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _ci, _ci, _cf, _cf, _vp, _ci, _vp, _vp, _vp]
    ro, n_, il, pr, su = _hi(row_off), _hi(n), _hi(is_last), _hi(pre), _hi(suf)
    _ck(lib.pfhip_op_cif_stream_fires(_p(enc), enc.stride(0), _p(alphas), ro[1], n_[1], il[1], pr[1], su[1], _p(carry), carry.stride(0), B,
                                      D, float(threshold), float(tail), _p(emb), emb.shape[1], _p(n_fire), _p(fire_step), _stream()),
        "cif_stream_fires")


def fsmn_cached(t2, w, res, out, tok_off, n_tok, dcache, layer):
    """The streaming decoder's cached FSMN for B connections: out (may be res) = res + t2 + conv over [cache; t2];
    dcache [B, layers, 10, C] is advanced in place.  tok_off / n_tok: host int sequences."""
    lib = _lib()
    lib.pfhip_op_fsmn_cached.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _ci, _ci, _ci, _vp]
    to, nt = _hi(tok_off), _hi(n_tok)
    _ck(lib.pfhip_op_fsmn_cached(_p(t2), _p(w), _p(res), _p(out), to[1], nt[1], _p(dcache), dcache.stride(0), len(n_tok), layer,
                                 t2.shape[1], _stream()), "fsmn_cached")


def fsmn_causal20(p, w, row_off, T, final, cache_in, cache_out, layer, C, out):
    """The FSMN-VAD memory block (left order 20) for B connections: out rows = p + causal conv over [cache_in; p]; cache_out
    [B, layers, 19, C] receives the last 19 rows of [cache_in; p] where final[b] == 0.  row_off / T / final: host int sequences."""
    lib = _lib()
    lib.pfhip_op_fsmn_causal20.argtypes = [_vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _ci, _ci, _vp, _ci, _ci, _vp]
    ro, tt, fi = _hi(row_off), _hi(T), _hi(final)
    _ck(lib.pfhip_op_fsmn_causal20(_p(p), p.stride(0), _p(w), ro[1], tt[1], fi[1], _p(cache_in), _p(cache_out), cache_in.stride(0), len(T),
                                   layer, _p(out), out.stride(0), C, _stream()), "fsmn_causal20")


def softmax_rows(x, M, N, y, col0=None):
    """y [>= M, N] = softmax over columns [0, N) of x's rows; col0 [>= M] (optional) = y[:, 0]."""
    lib = _lib()
    lib.pfhip_op_softmax_rows.argtypes = [_vp, _ci, _ci, _ci, _vp, _vp, _vp]
    _ck(lib.pfhip_op_softmax_rows(_p(x), x.stride(0), M, N, _p(y), _p(col0), _stream()), "softmax_rows")


def im2col3(h, row_pos, row_len, D, ldc=None, out=None):
    """col [M, 3 D] = [h[row - 1] | h[row] | h[row + 1]] with zeros outside the row's utterance (row_pos / row_len: int32 device)."""
    M = row_pos.numel()
    col = out if out is not None else torch.empty((M, 3 * D if ldc is None else ldc), dtype=torch.float32, device=h.device)
    lib = _lib()
    lib.pfhip_op_im2col3.argtypes = [_vp, _ci, _vp, _ci, _vp, _vp, _ci, _ci, _vp]
    _ck(lib.pfhip_op_im2col3(_p(h), h.stride(0), _p(col), col.stride(0), _p(row_pos), _p(row_len), M, D, _stream()), "im2col3")
    return col


def alpha(o, w, b, smooth, noise, M, D):
    lib = _lib()
    lib.pfhip_op_alpha.argtypes = [_vp, _ci, _vp, _vp, _cf, _cf, _vp, _ci, _ci, _vp]
    a = torch.empty(M, dtype=torch.float32, device=o.device)
    _ck(lib.pfhip_op_alpha(_p(o), o.stride(0), _p(w), _p(b), float(smooth), float(noise), _p(a), M, D, _stream()), "alpha")
    return a


def alpha2(y, w, b, smooth, noise, M, D):
    lib = _lib()
    lib.pfhip_op_alpha2.argtypes = [_vp, _ci, _vp, _cf, _cf, _cf, _vp, _ci, _ci, _vp]
    a = torch.empty(M, dtype=torch.float32, device=y.device)
    _ck(lib.pfhip_op_alpha2(_p(y), y.stride(0), _p(w), float(b), float(smooth), float(noise), _p(a), M, D, _stream()), "alpha2")
    return a


def us_cif(a2, off, length, token_num, threshold):
    """(us_alphas, us_peaks) of the timestamp head for the utterances (off, length, token_num: int32 device tensors)."""
    lib = _lib()
    lib.pfhip_op_us_cif.argtypes = [_vp, _vp, _vp, _vp, _ci, _ci, _cf, _vp, _vp, _vp]
    us_alphas, us_peaks = torch.zeros_like(a2), torch.zeros_like(a2)
    _ck(lib.pfhip_op_us_cif(_p(a2), _p(off), _p(length), _p(token_num), off.numel(), int(length.max().item()), float(threshold),
                            _p(us_alphas), _p(us_peaks), _stream()), "us_cif")
    return us_alphas, us_peaks


def blstm_scratch():
    """(floats of scratch pfhip_op_blstm takes, index of its error word): the layout csrc/kernels.h states, asked of the library."""
    lib = _lib()
    return int(lib.pfhip_op_blstm_scratch_floats()), int(lib.pfhip_op_blstm_flag_word())


def blstm_entry(gx, whh, y, off, length, B, Lmax, stepwise, hx, cst):
    """pfhip_op_blstm as it is, on the current stream, nothing allocated or checked here (any tensor may be None = NULL)."""
    lib = _lib()
    lib.pfhip_op_blstm.argtypes = [_vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _vp, _vp, _vp]
    _ck(lib.pfhip_op_blstm(_p(gx), _p(whh), _p(y), _p(off), _p(length), int(B), int(Lmax), int(bool(stepwise)), _p(hx), _p(cst), _stream()),
        "blstm")


def blstm(gx, whh, off, length, stepwise=False, Lmax=None, y=None):
    """The timestamp head's BLSTM recurrence: gx [rows, 4096], whh [2, 2048, 512], off / length int32 device tensors of B <= 32
    utterances.  stepwise=False runs the persistent kernel, True the one-launch-per-step form.  Runs on the current stream and
    synchronises.  Returns (y [rows, 1024], flag, xcc_words): flag is the persistent kernel's error word (0 = served, 1 = the h
    exchange timed out, 2 = a direction's blocks were not on one XCD), xcc_words the XCC id + 1 each direction noted (0 = never
    written; the stepwise form writes neither).  A y that is passed in is written in place, rows outside utterances untouched."""
    B = off.numel()
    if Lmax is None:
        Lmax = int(length.max().item()) if B else 0
    if y is None:
        y = torch.zeros((gx.shape[0], 1024), dtype=torch.float32, device=gx.device)
    n_scratch, flag_word = blstm_scratch()
    hx = torch.zeros(n_scratch, dtype=torch.float32, device=gx.device)
    cst = torch.zeros(2 * 32 * 512, dtype=torch.float32, device=gx.device)
    blstm_entry(gx, whh, y, off, length, B, Lmax, stepwise, hx, cst)
    torch.cuda.current_stream().synchronize()
    state = hx[flag_word:flag_word + 4].view(torch.int32).cpu().tolist()
    return y, state[0], (state[2], state[3])


def lstm_cell(G, c, h, lens, t, sel):
    """One LSTM step in place on c, h [H, D] from pre-activations G [H, 4 D]; sel rows with lens - 1 == t receive h."""
    H, D = c.shape
    lib = _lib()
    lib.pfhip_op_lstm_cell.argtypes = [_vp, _vp, _vp, _vp, _ci, _vp, _ci, _ci, _vp]
    _ck(lib.pfhip_op_lstm_cell(_p(G), _p(c), _p(h), _p(lens), int(t), _p(sel), H, D, _stream()), "lstm_cell")


def frame_energy(pcm, sample_off, n_samples, flen=400, fshift=160):
    """Frame energies sum x^2 (25-ms windows at a 10-ms shift by default) of the utterances packed in `pcm`, a float32 or int16 device
    tensor (int16 means s / 32768): utterance b is n_samples[b] samples from sample_off[b] (host int sequences).  Returns
    (e, frame_off): e float32 [total frames] on the device, utterance b's frames at e[frame_off[b]:frame_off[b + 1]]."""
    lib = _lib()
    lib.pfhip_op_frame_energy.argtypes = [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp]
    lib.pfhip_op_frame_energy_s16.argtypes = lib.pfhip_op_frame_energy.argtypes
    nf = [0 if n < flen else 1 + (n - flen) // fshift for n in n_samples]
    fo = [0]
    for f in nf:
        fo.append(fo[-1] + f)
    dev = pcm.device
    d_so = torch.tensor(list(sample_off), dtype=torch.int64, device=dev)
    d_fo = torch.tensor(fo, dtype=torch.int32, device=dev)
    d_nf = torch.tensor(nf, dtype=torch.int32, device=dev)
    e = torch.empty(max(fo[-1], 1), dtype=torch.float32, device=dev)
    if pcm.dtype not in (torch.float32, torch.int16):
        raise PfhipError("frame_energy takes float32 or int16 samples")
    fn = lib.pfhip_op_frame_energy_s16 if pcm.dtype == torch.int16 else lib.pfhip_op_frame_energy
    _ck(fn(_p(pcm), _p(d_so), _p(d_fo), _p(d_nf), len(nf), fo[-1], int(flen), int(fshift), _p(e), _stream()), "frame_energy")
    return e[:fo[-1]], fo


# ---- the front-end kernels, the LFR/CMVN family, the PE kernels, the gathers and small reductions ------------------------------------
def _hl(values):
    """_hi for int64 host arrays."""
    import numpy as np
    a = np.ascontiguousarray(values, np.int64)
    return a, ctypes.c_void_p(a.ctypes.data)


def fbank_entry(pcm, pcm_samples, sample_off, frame_off, nframes, B, total_frames, fb_out=None, feats=None, feats_rows=0, row_off=None,
                cmvn_mean=None, cmvn_istd=None):
    """pfhip_op_fbank / pfhip_op_fbank_s16 (by pcm's dtype, float32 or int16) as it is: nothing derived or checked here.  sample_off /
    frame_off / nframes / row_off: host int sequences or None (= NULL)."""
    lib = _lib()
    lib.pfhip_op_fbank.argtypes = [_vp, _ll, _vp, _vp, _vp, _ci, _ci, _vp, _vp, _ll, _vp, _vp, _vp, _vp]
    lib.pfhip_op_fbank_s16.argtypes = lib.pfhip_op_fbank.argtypes
    if pcm is not None and pcm.dtype not in (torch.float32, torch.int16):
        raise PfhipError("fbank takes float32 or int16 samples")
    fn = lib.pfhip_op_fbank_s16 if pcm is not None and pcm.dtype == torch.int16 else lib.pfhip_op_fbank
    so = _hl(sample_off) if sample_off is not None else (None, None)
    fo = _hi(frame_off) if frame_off is not None else (None, None)
    nf = _hi(nframes) if nframes is not None else (None, None)
    ro = _hi(row_off) if row_off is not None else (None, None)
    _ck(fn(_p(pcm), int(pcm_samples), so[1], fo[1], nf[1], int(B), int(total_frames), _p(fb_out), _p(feats), int(feats_rows), ro[1],
           _p(cmvn_mean), _p(cmvn_istd), _stream()), "fbank")


def fbank_layout(n_samples, flen=400, fshift=160):
    """(nframes, frame_off) of utterances of n_samples[b] samples: what the fbank entries take."""
    nf = [0 if n < flen else 1 + (n - flen) // fshift for n in n_samples]
    fo = [0]
    for f in nf:
        fo.append(fo[-1] + f)
    return nf, fo


def fbank_frames(pcm, sample_off, n_samples, out):
    """Raw log-mel frames of the utterances packed in `pcm` (float32 or int16 device tensor; utterance b is n_samples[b] samples from
    sample_off[b], host int sequences) into out [>= total frames, 80].  Returns frame_off."""
    nf, fo = fbank_layout(n_samples)
    fbank_entry(pcm, pcm.numel(), sample_off, fo, nf, len(nf), fo[-1], fb_out=out)
    return fo


def fbank_lfr_cmvn(pcm, sample_off, n_samples, row_off, cmvn_mean, cmvn_istd, feats):
    """The fused form: LFR (7, 6) + CMVN rows of utterance b at row row_off[b] of feats [rows, 560]."""
    nf, fo = fbank_layout(n_samples)
    fbank_entry(pcm, pcm.numel(), sample_off, fo, nf, len(nf), fo[-1], feats=feats, feats_rows=feats.shape[0], row_off=row_off,
                cmvn_mean=cmvn_mean, cmvn_istd=cmvn_istd)
    return fo


def lfr_cmvn(fb, F, m, n, n_mels, mean, istd, out):
    """out [>= ceil(F / n), ldo] = LfrCmvn of fb [F, n_mels]; columns m * n_mels .. ldo zeroed."""
    lib = _lib()
    lib.pfhip_op_lfr_cmvn.argtypes = [_vp, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _ci, _vp]
    _ck(lib.pfhip_op_lfr_cmvn(_p(fb), int(F), int(m), int(n), int(n_mels), _p(mean), _p(istd), _p(out), out.stride(0), _stream()), "lfr_cmvn")


def lfr_cmvn_packed(fb, frame_off, nframes, row_off, m, n, n_mels, mean, istd, out):
    """LfrCmvn of the files packed in fb [frames, n_mels] (frame_off / nframes / row_off: host int sequences)."""
    lib = _lib()
    lib.pfhip_op_lfr_cmvn_packed.argtypes = [_vp, _ll, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _ci, _ll, _vp]
    fo, nf, ro = _hi(frame_off), _hi(nframes), _hi(row_off)
    _ck(lib.pfhip_op_lfr_cmvn_packed(_p(fb), fb.shape[0], fo[1], nf[1], ro[1], len(nframes), int(m), int(n), int(n_mels), _p(mean), _p(istd),
                                     _p(out), out.stride(0), out.shape[0], _stream()), "lfr_cmvn_packed")


def lfr_cmvn_online_batch(fb, fb_off, Tin, n_out, row_off, m, n, n_mels, mean, istd, out):
    """OnlineLfrCmvn rows of many connections (fb_off / Tin / n_out / row_off: host int sequences, in frames and rows)."""
    lib = _lib()
    lib.pfhip_op_lfr_cmvn_online_batch.argtypes = [_vp, _ll, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _ci, _ll, _vp]
    fo, ti, no, ro = _hi(fb_off), _hi(Tin), _hi(n_out), _hi(row_off)
    _ck(lib.pfhip_op_lfr_cmvn_online_batch(_p(fb), fb.shape[0], fo[1], ti[1], no[1], ro[1], len(Tin), int(m), int(n), int(n_mels), _p(mean),
                                           _p(istd), _p(out), out.stride(0), out.shape[0], _stream()), "lfr_cmvn_online_batch")


def stream_lfr_batch(fb, fb_off, T, n_rows, pos0, row_off, mean, istd, scale, inv_ts, out):
    """The streaming front end's LFR + CMVN + scale + PE rows of many connections into out [rows, ldo >= 560]."""
    lib = _lib()
    lib.pfhip_op_stream_lfr_batch.argtypes = [_vp, _ll, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _cf, _vp, _vp, _ci, _ll, _vp]
    fo, tt, nr, p0, ro = _hi(fb_off), _hi(T), _hi(n_rows), _hi(pos0), _hi(row_off)
    _ck(lib.pfhip_op_stream_lfr_batch(_p(fb), fb.shape[0], fo[1], tt[1], nr[1], p0[1], ro[1], len(T), _p(mean), _p(istd), float(scale),
                                      _p(inv_ts), _p(out), out.stride(0), out.shape[0], _stream()), "stream_lfr_batch")


def rows_copy_batch(dst, dst_off, src, src_off, ldd, lds, nrows, ncols):
    """Many row copies in one launch over flat float32 tensors dst / src (src may be None); a negative src_off means zeros."""
    lib = _lib()
    lib.pfhip_op_rows_copy_batch.argtypes = [_vp, _ll, _vp, _vp, _ll, _vp, _vp, _vp, _vp, _vp, _ci, _vp]
    do, so, a, b, c, d = _hl(dst_off), _hl(src_off), _hi(ldd), _hi(lds), _hi(nrows), _hi(ncols)
    _ck(lib.pfhip_op_rows_copy_batch(_p(dst), dst.numel(), do[1], _p(src), src.numel() if src is not None else 0, so[1], a[1], b[1], c[1],
                                     d[1], len(nrows), _stream()), "rows_copy_batch")


def embed(feats, D, x0, row_pos, M, inv_ts, scale):
    """x0 [>= M, ldx] = feats [M, D] * scale + PE(row_pos + 1); columns D .. ldx zeroed."""
    lib = _lib()
    lib.pfhip_op_embed.argtypes = [_vp, _ci, _vp, _ci, _vp, _ci, _vp, _cf, _vp]
    _ck(lib.pfhip_op_embed(_p(feats), int(D), _p(x0), x0.stride(0), _p(row_pos), int(M), _p(inv_ts), float(scale), _stream()), "embed")


def embed_gather(ids, table, D, Dout, out, N, inv_ts, scale, pos_of_row=None):
    """out [>= N, ldo] = table[clamped id] * scale + PE; columns D .. Dout zeroed."""
    lib = _lib()
    lib.pfhip_op_embed_gather.argtypes = [_vp, _vp, _ci, _ci, _ci, _vp, _ci, _ci, _vp, _cf, _vp, _vp]
    _ck(lib.pfhip_op_embed_gather(_p(ids), _p(table), table.shape[0], int(D), int(Dout), _p(out), out.stride(0), int(N), _p(inv_ts),
                                  float(scale), _p(pos_of_row), _stream()), "embed_gather")


def argmax_first(logits, N, ncls, out):
    lib = _lib()
    lib.pfhip_op_argmax_first.argtypes = [_vp, _ci, _ci, _ci, _vp, _vp]
    _ck(lib.pfhip_op_argmax_first(_p(logits), logits.stride(0), int(N), int(ncls), _p(out), _stream()), "argmax_first")


def compact(stage, emb, src_row, ML, D):
    lib = _lib()
    lib.pfhip_op_compact.argtypes = [_vp, _vp, _vp, _ci, _ci, _vp]
    _ck(lib.pfhip_op_compact(_p(stage), _p(emb), _p(src_row), int(ML), int(D), _stream()), "compact")


def gather_rows(ids, table, D, out, R):
    lib = _lib()
    lib.pfhip_op_gather_rows.argtypes = [_vp, _vp, _ci, _vp, _ci, _vp]
    _ck(lib.pfhip_op_gather_rows(_p(ids), _p(table), int(D), _p(out), int(R), _stream()), "gather_rows")


def svs_prompt_rows(E, D, prompt, row_off, length, B, feats):
    lib = _lib()
    lib.pfhip_op_svs_prompt_rows.argtypes = [_vp, _ci, _vp, _vp, _vp, _ci, _vp, _ci, _vp]
    _ck(lib.pfhip_op_svs_prompt_rows(_p(E), int(D), _p(prompt), _p(row_off), _p(length), int(B), _p(feats), feats.stride(0), _stream()),
        "svs_prompt_rows")


def gather_best(logp, ids, M, best):
    lib = _lib()
    lib.pfhip_op_gather_best.argtypes = [_vp, _ci, _vp, _ci, _vp, _vp]
    _ck(lib.pfhip_op_gather_best(_p(logp), logp.stride(0), _p(ids), int(M), _p(best), _stream()), "gather_best")


def row_lse(logits, M, V, lse):
    lib = _lib()
    lib.pfhip_op_row_lse.argtypes = [_vp, _ci, _ci, _ci, _vp, _vp]
    _ck(lib.pfhip_op_row_lse(_p(logits), logits.stride(0), int(M), int(V), _p(lse), _stream()), "row_lse")


# ---- the DNSMOS networks' kernels (csrc/conv3x3.hip, csrc/dnsmos.hip) ----------------------------------------------------------------
def conv3x3_relu(x, w, bias, pool=False, out=None):
    """Conv 3x3 / pad 1 / stride 1 + bias + ReLU (+ the 2x2 floor max-pool) on NHWC float32: x [N, H, W, Cin] ([N, H, W] for Cin == 1),
    w the ONNX [Cout, Cin, 3, 3], bias [Cout] -> [N, H, W, Cout], pooled [N, H // 2, W // 2, Cout].  `out`: a float32 device tensor
    with room for the result (tests pass one with a canary behind it)."""
    lib = _lib()
    lib.pfhip_op_conv3x3_relu.argtypes = [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp]
    Cout, Cin = int(w.shape[0]), int(w.shape[1])
    N, H, W = (int(v) for v in x.shape[:3])
    if not (x.is_contiguous() and w.is_contiguous() and bias.is_contiguous()) or x.numel() != N * H * W * Cin:
        raise PfhipError("conv3x3_relu takes contiguous NHWC activations and ONNX-layout weights")
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    if out is None:
        out = torch.empty((N, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    elif out.numel() < N * Ho * Wo * Cout:
        raise PfhipError("conv3x3_relu: out is too small")
    _ck(lib.pfhip_op_conv3x3_relu(_p(x), _p(w), _p(bias), _p(out), N, H, W, Cin, Cout, 1 if pool else 0, _stream()), "conv3x3_relu")
    return out


def dnsmos_logpow(pcm, win_off, stft_real, stft_imag, n_frames=900, floor=1e-12, power=2.0, denom=2.3025851, out=None):
    """The primary DNSMOS net's front end: pcm a float32 or int16 device tensor (int16 means s / 32768), window i the 160 * (n_frames + 1)
    samples from win_off[i] (host ints); stft_real / stft_imag the graph's kernels [161, 320(, 1)]; floor / power / denom its three
    scalar initialisers.  Returns [n_win, n_frames, 161]."""
    lib = _lib()
    lib.pfhip_op_dnsmos_logpow.argtypes = [_vp, ctypes.c_longlong, _vp, _ci, _ci, _vp, _vp, _cf, _cf, _cf, _vp, _vp]
    lib.pfhip_op_dnsmos_logpow_s16.argtypes = lib.pfhip_op_dnsmos_logpow.argtypes
    if pcm.dtype not in (torch.float32, torch.int16):
        raise PfhipError("dnsmos_logpow takes float32 or int16 samples")
    if stft_real.numel() != 161 * 320 or stft_imag.numel() != 161 * 320:
        raise PfhipError("dnsmos_logpow: the STFT kernels are [161, 320]")
    off, off_p = _hl(win_off)
    if out is None:
        out = torch.empty((len(off), n_frames, 161), dtype=torch.float32, device=pcm.device)
    elif out.numel() < len(off) * n_frames * 161:
        raise PfhipError("dnsmos_logpow: out is too small")
    fn = lib.pfhip_op_dnsmos_logpow_s16 if pcm.dtype == torch.int16 else lib.pfhip_op_dnsmos_logpow
    _ck(fn(_p(pcm), pcm.numel(), off_p, len(off), int(n_frames), _p(stft_real), _p(stft_imag), float(floor), float(power), float(denom),
           _p(out), _stream()), "dnsmos_logpow")
    return out


def dnsmos_melspec(pcm, win_off, out=None):
    """The P.808 DNSMOS net's input (dnsmos_local.py's audio_melspec; librosa's defaults recalled, see pfhip_ops.h): window i the
    144000 samples from win_off[i] of the float32 / int16 device tensor pcm.  Returns [n_win, 900, 120]."""
    lib = _lib()
    lib.pfhip_op_dnsmos_melspec.argtypes = [_vp, ctypes.c_longlong, _vp, _ci, _vp, _vp]
    lib.pfhip_op_dnsmos_melspec_s16.argtypes = lib.pfhip_op_dnsmos_melspec.argtypes
    if pcm.dtype not in (torch.float32, torch.int16):
        raise PfhipError("dnsmos_melspec takes float32 or int16 samples")
    off, off_p = _hl(win_off)
    if out is None:
        out = torch.empty((len(off), 900, 120), dtype=torch.float32, device=pcm.device)
    elif out.numel() < len(off) * 900 * 120:
        raise PfhipError("dnsmos_melspec: out is too small")
    fn = lib.pfhip_op_dnsmos_melspec_s16 if pcm.dtype == torch.int16 else lib.pfhip_op_dnsmos_melspec
    _ck(fn(_p(pcm), pcm.numel(), off_p, len(off), _p(out), _stream()), "dnsmos_melspec")
    return out


def globalmax_mlp(x, w1, b1, w2, b2, w3, b3, out=None):
    """Global max over H and W of x [N, H, W, C], then three dense layers y = x @ w + b (w [in, out], as the graph's MatMul holds it)
    with ReLU after the first two.  Returns [N, D3]."""
    lib = _lib()
    lib.pfhip_op_globalmax_mlp.argtypes = [_vp, _ci, _ci, _ci, _vp, _vp, _ci, _vp, _vp, _ci, _vp, _vp, _ci, _vp, _vp]
    N, H, W, C = (int(v) for v in x.shape)
    if not all(t.is_contiguous() for t in (x, w1, b1, w2, b2, w3, b3)):
        raise PfhipError("globalmax_mlp takes contiguous tensors")
    if w1.shape[0] != C or w2.shape[0] != w1.shape[1] or w3.shape[0] != w2.shape[1]:
        raise PfhipError("globalmax_mlp: the dense layers do not chain")
    D1, D2, D3 = int(w1.shape[1]), int(w2.shape[1]), int(w3.shape[1])
    if out is None:
        out = torch.empty((N, D3), dtype=torch.float32, device=x.device)
    elif out.numel() < N * D3:
        raise PfhipError("globalmax_mlp: out is too small")
    _ck(lib.pfhip_op_globalmax_mlp(_p(x), N, H * W, C, _p(w1), _p(b1), D1, _p(w2), _p(b2), D2, _p(w3), _p(b3), D3, _p(out), _stream()),
        "globalmax_mlp")
    return out
