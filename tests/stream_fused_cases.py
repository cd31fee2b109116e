"""The case table of the one-window fused launches (csrc/stream_fused.hip), shared by test_stream_fused_routes.py (CPU: the table
reaches every route) and test_gpu_stream_fused_routes.py (GPU: every case against an exact and an fp64 reference).

A route is what the launcher's own route function (ops.fused_gemv_1trip_route / ops.fused_ln_gemm_route) answers for a shape: the
kernel instantiation, the wave count and how the k-blocks fall on the waves.  Nothing here decides a route: the ids are spelled from
the functions' answers, and the table below is what `python tests/stream_fused_cases.py` prints (CPU; needs the built library).
"""
from collections import namedtuple

# form: "1trip" | "ln_gemm"; the route is the same for every M in [m_lo, m_hi] of the reachable grid (both ends run on the GPU)
Case = namedtuple("Case", "route form m_lo m_hi N K ln fsmn")

KNOBS = ("PFHIP_STREAM_1TRIP", "PFHIP_1T_CPL", "PFHIP_STREAM_FUSED_MFMA")      # they change the dispatch: the tests refuse to run under them

GRID_M = (1, 8, 9, 16, 17, 20, 21, 24, 25, 32)
# 7 / 8: ragged / whole against 2- and 4-column patches; 644 / 648: against 8; 4100 / 4104: against 32; both sides of 640 and 4096
GRID_N = (7, 8, 636, 640, 644, 648, 4092, 4096, 4100, 4104)
GRID_K = tuple(sorted(set(range(64, 4097, 64)) | {96, 544}))
LN_GEMM_MAX_D = 2048          # pfhip_op_fused_ln_gemm refuses a LayerNorm wider than this, and D pads to K within one k-block


def route_1trip(ops, M, N, K, ln, fsmn):
    """Route id of the one-trip form, None where it refuses the shape."""
    r = ops.fused_gemv_1trip_route(M, N, K, ln, fsmn)
    if not r["ok"]:
        return None
    kind = "ln" if r["ln"] else "fs" if r["fs"] else "pl"
    return f"1t-{kind}-cw{r['cw']}x{r['cpl']}-r{r['rpl']}-nf{r['nf']}-w{r['waves']}"


def route_ln_gemm(ops, M, N, K, ln):
    """Route id of fused_ln_gemm: the instantiation, the waves, and the trips a wave makes through its k-blocks (vector form: 1, 2,
    3 or more; matrix form: fewer than 4 = only the single-step loop, a multiple of 4 = only the unrolled one, 5 = both), `r` where
    the k-blocks do not fill the waves evenly."""
    r = ops.fused_ln_gemm_route(M, N, K, ln)
    trips = -(-r["k_blocks"] // r["waves"])
    ragged = "r" if r["k_blocks"] % r["waves"] else ""
    kind = "ln" if r["ln"] else "pl"
    if r["kernel"] == "vector":
        return f"vec-{kind}-cw{r['cw']}-mr{r['mr']}-w{r['waves']}-k{min(trips, 3)}{ragged}"
    assert r["kernel"] == "matrix", r
    return f"mat-{kind}-cw{r['cw']}-k{1 if trips < 4 else 4 if trips % 4 == 0 else 5}{ragged}"


def route_of(ops, form, M, N, K, ln, fsmn):
    return route_1trip(ops, M, N, K, ln, fsmn) if form == "1trip" else route_ln_gemm(ops, M, N, K, ln)


def production_calls(cfg):
    """Every launch stream.cpp makes on the lean path for a model of these widths: (name, rows, N, K, ln, fsmn, fallback) with rows
    "window" (M) or "token" (ML), the one-trip form first where the call site tries it (one_trip) and fused_ln_gemm where it falls."""
    d, ffn, dffn = cfg["d_model"], cfg["ffn"], cfg["dec_ffn"]
    feat_pad = (cfg["n_mels"] * cfg["lfr_m"] + 31) // 32 * 32
    kv = cfg["dec_layers"] * 2 * d
    Call = namedtuple("Call", "name rows N K ln fsmn one_trip ln_gemm")
    return [
        Call("enc0.qkv", "window", 3 * d, feat_pad, True, False, False, True),       # layer 0 has no folded weight
        Call("enc.qkv", "window", 3 * d, d, True, False, True, True),
        Call("enc.out+fsmn", "window", d, d, False, True, True, True),
        Call("enc.ffn1", "window", ffn, d, True, False, True, True),
        Call("enc.ffn2", "window", d, ffn, False, False, True, True),
        Call("pred.conv", "window", d, 3 * d, False, False, True, False),            # falls to the general GEMM
        Call("dec.ffn1", "token", dffn, d, True, False, True, True),
        Call("dec.ffn2'", "token", d, dffn, True, False, True, True),
        Call("dec.q", "token", d, d, True, False, True, True),
        Call("dec.kv_all", "window", kv, d, False, False, True, True),
        Call("dec.out", "token", d, d, False, False, True, True),
        Call("dec.vocab", "token", cfg["vocab"], d, True, False, False, True),
    ]


def production_grid(ops, weights):
    """(form, M, N, K, ln, fsmn, route) of every launch of both served widths with 1..32 rows, each call falling from the one-trip
    form to fused_ln_gemm as gemv1 / ln_gemm do."""
    out = []
    for cfg in (weights.PARAFORMER_LARGE, weights.PARAFORMER_SMALL):
        for c in production_calls(cfg):
            for M in range(1, 33):
                r = route_1trip(ops, M, c.N, c.K, c.ln, c.fsmn) if c.one_trip else None
                if r is not None:
                    out.append(("1trip", M, c.N, c.K, c.ln, c.fsmn, r))
                elif c.ln_gemm:
                    out.append(("ln_gemm", M, c.N, c.K, c.ln, c.fsmn, route_ln_gemm(ops, M, c.N, c.K, c.ln)))
    return out


_reachable = []


def reachable_grid(ops):
    """The same tuples for every shape of GRID_M x GRID_N x GRID_K, LayerNorm and FSMN on and off, given to both entries."""
    if _reachable:
        return _reachable
    out = _reachable
    for N in GRID_N:
        for K in GRID_K:
            for ln in (False, True):
                for M in GRID_M:
                    for fsmn in (False, True):
                        r = route_1trip(ops, M, N, K, ln, fsmn)
                        if r is not None:
                            out.append(("1trip", M, N, K, ln, fsmn, r))
                    if not (ln and K > LN_GEMM_MAX_D):
                        out.append(("ln_gemm", M, N, K, ln, False, route_ln_gemm(ops, M, N, K, ln)))
    return out


def representatives(ops):
    """One case per route of the reachable grid: the first shape in the grid's order (smallest N, then K) that takes it, with the
    lowest and the highest M of GRID_M that take it at that shape."""
    first = {}
    for form, M, N, K, ln, fsmn, r in reachable_grid(ops):
        if r not in first:
            first[r] = [form, M, M, N, K, ln, fsmn]
        elif first[r][3:] == [N, K, ln, fsmn]:
            first[r][2] = max(first[r][2], M)
    return [Case(r, *v) for r, v in sorted(first.items())]


# Shapes kept by name, whatever the representatives are: the defects this table found, the issue's known answers, served shapes.
PINNED = [
    # K % 128 == 64 at N <= 640: the 2-column vector form (k-block 128) dropped the last 64 columns of K
    Case("vec-pl-cw4-mr24-w16-k2r", "ln_gemm", 20, 20, 512, 1088, False, False),
    Case("vec-ln-cw4-mr32-w16-k2r", "ln_gemm", 25, 25, 512, 1088, True, False),
    # K = 64 without LayerNorm: one or two waves were fewer threads than the MR x CW outputs a workgroup finishes
    Case("vec-pl-cw4-mr24-w2-k1r", "ln_gemm", 17, 24, 7, 64, False, False),
    Case("vec-pl-cw8-mr32-w4-k1r", "ln_gemm", 25, 32, 644, 64, False, False),
    # the served shapes of the issue's list
    Case("1t-pl-cw4x2-r5-nf3-w16", "1trip", 20, 20, 512, 1536, False, False),       # predictor conv, large model
    Case("1t-ln-cw4x2-r5-nf4-w10", "1trip", 20, 20, 320, 1280, True, False),        # small model's folded decoder FFN2
    Case("vec-ln-cw8-mr24-w16-k1r", "ln_gemm", 20, 20, 960, 320, True, False),      # small model's QKV: 20 waves refused by the one-trip form
    Case("vec-ln-cw2-mr32-w16-k1", "ln_gemm", 25, 25, 512, 2048, True, False),      # a decoder window of 25 tokens, folded FFN2
    Case("mat-ln-cw32-k4", "ln_gemm", 20, 20, 8404, 512, True, False),              # vocabulary projection
]

# python tests/stream_fused_cases.py prints this list
REPRESENTATIVES = [
    Case("1t-fs-cw2x2-r2-nf2-w16", "1trip", 1, 8, 8, 2048, False, True),
    Case("1t-fs-cw2x2-r2-nf3-w16", "1trip", 1, 8, 8, 3072, False, True),
    Case("1t-fs-cw2x2-r2-nf4-w16", "1trip", 1, 8, 8, 4096, False, True),
    Case("1t-fs-cw2x2-r5-nf2-w16", "1trip", 9, 20, 8, 2048, False, True),
    Case("1t-fs-cw2x2-r5-nf3-w16", "1trip", 9, 20, 8, 3072, False, True),
    Case("1t-fs-cw2x2-r5-nf4-w16", "1trip", 9, 20, 8, 4096, False, True),
    Case("1t-fs-cw4x2-r2-nf1-w2", "1trip", 1, 8, 8, 64, False, True),
    Case("1t-fs-cw4x2-r2-nf1-w3", "1trip", 1, 8, 8, 96, False, True),
    Case("1t-fs-cw4x2-r2-nf2-w10", "1trip", 1, 8, 8, 640, False, True),
    Case("1t-fs-cw4x2-r2-nf2-w11", "1trip", 1, 8, 8, 704, False, True),
    Case("1t-fs-cw4x2-r2-nf2-w12", "1trip", 1, 8, 8, 768, False, True),
    Case("1t-fs-cw4x2-r2-nf2-w13", "1trip", 1, 8, 8, 832, False, True),
    Case("1t-fs-cw4x2-r2-nf2-w14", "1trip", 1, 8, 8, 896, False, True),
    Case("1t-fs-cw4x2-r2-nf2-w15", "1trip", 1, 8, 8, 960, False, True),
    Case("1t-fs-cw4x2-r2-nf2-w2", "1trip", 1, 8, 8, 128, False, True),
    Case("1t-fs-cw4x2-r2-nf2-w3", "1trip", 1, 8, 8, 192, False, True),
    Case("1t-fs-cw4x2-r2-nf2-w4", "1trip", 1, 8, 8, 256, False, True),
    Case("1t-fs-cw4x2-r2-nf2-w5", "1trip", 1, 8, 8, 320, False, True),
    Case("1t-fs-cw4x2-r2-nf2-w6", "1trip", 1, 8, 8, 384, False, True),
    Case("1t-fs-cw4x2-r2-nf2-w7", "1trip", 1, 8, 8, 448, False, True),
    Case("1t-fs-cw4x2-r2-nf2-w8", "1trip", 1, 8, 8, 512, False, True),
    Case("1t-fs-cw4x2-r2-nf2-w9", "1trip", 1, 8, 8, 576, False, True),
    Case("1t-fs-cw4x2-r2-nf3-w16", "1trip", 1, 8, 8, 1536, False, True),
    Case("1t-fs-cw4x2-r2-nf4-w10", "1trip", 1, 8, 8, 1280, False, True),
    Case("1t-fs-cw4x2-r2-nf4-w11", "1trip", 1, 8, 8, 1408, False, True),
    Case("1t-fs-cw4x2-r2-nf4-w8", "1trip", 1, 8, 8, 1024, False, True),
    Case("1t-fs-cw4x2-r2-nf4-w9", "1trip", 1, 8, 8, 1152, False, True),
    Case("1t-fs-cw4x2-r5-nf1-w2", "1trip", 9, 20, 8, 64, False, True),
    Case("1t-fs-cw4x2-r5-nf1-w3", "1trip", 9, 20, 8, 96, False, True),
    Case("1t-fs-cw4x2-r5-nf2-w10", "1trip", 9, 20, 8, 640, False, True),
    Case("1t-fs-cw4x2-r5-nf2-w11", "1trip", 9, 20, 8, 704, False, True),
    Case("1t-fs-cw4x2-r5-nf2-w12", "1trip", 9, 20, 8, 768, False, True),
    Case("1t-fs-cw4x2-r5-nf2-w13", "1trip", 9, 20, 8, 832, False, True),
    Case("1t-fs-cw4x2-r5-nf2-w14", "1trip", 9, 20, 8, 896, False, True),
    Case("1t-fs-cw4x2-r5-nf2-w15", "1trip", 9, 20, 8, 960, False, True),
    Case("1t-fs-cw4x2-r5-nf2-w2", "1trip", 9, 20, 8, 128, False, True),
    Case("1t-fs-cw4x2-r5-nf2-w3", "1trip", 9, 20, 8, 192, False, True),
    Case("1t-fs-cw4x2-r5-nf2-w4", "1trip", 9, 20, 8, 256, False, True),
    Case("1t-fs-cw4x2-r5-nf2-w5", "1trip", 9, 20, 8, 320, False, True),
    Case("1t-fs-cw4x2-r5-nf2-w6", "1trip", 9, 20, 8, 384, False, True),
    Case("1t-fs-cw4x2-r5-nf2-w7", "1trip", 9, 20, 8, 448, False, True),
    Case("1t-fs-cw4x2-r5-nf2-w8", "1trip", 9, 20, 8, 512, False, True),
    Case("1t-fs-cw4x2-r5-nf2-w9", "1trip", 9, 20, 8, 576, False, True),
    Case("1t-fs-cw4x2-r5-nf3-w16", "1trip", 9, 20, 8, 1536, False, True),
    Case("1t-fs-cw4x2-r5-nf4-w10", "1trip", 9, 20, 8, 1280, False, True),
    Case("1t-fs-cw4x2-r5-nf4-w11", "1trip", 9, 20, 8, 1408, False, True),
    Case("1t-fs-cw4x2-r5-nf4-w8", "1trip", 9, 20, 8, 1024, False, True),
    Case("1t-fs-cw4x2-r5-nf4-w9", "1trip", 9, 20, 8, 1152, False, True),
    Case("1t-fs-cw8x2-r2-nf1-w12", "1trip", 1, 8, 648, 192, False, True),
    Case("1t-fs-cw8x2-r2-nf1-w16", "1trip", 1, 8, 648, 256, False, True),
    Case("1t-fs-cw8x2-r2-nf1-w4", "1trip", 1, 8, 648, 64, False, True),
    Case("1t-fs-cw8x2-r2-nf1-w6", "1trip", 1, 8, 648, 96, False, True),
    Case("1t-fs-cw8x2-r2-nf1-w8", "1trip", 1, 8, 648, 128, False, True),
    Case("1t-fs-cw8x2-r2-nf2-w16", "1trip", 1, 8, 648, 512, False, True),
    Case("1t-fs-cw8x2-r2-nf3-w16", "1trip", 1, 8, 648, 768, False, True),
    Case("1t-fs-cw8x2-r2-nf4-w16", "1trip", 1, 8, 648, 1024, False, True),
    Case("1t-fs-cw8x2-r5-nf1-w12", "1trip", 9, 20, 648, 192, False, True),
    Case("1t-fs-cw8x2-r5-nf1-w16", "1trip", 9, 20, 648, 256, False, True),
    Case("1t-fs-cw8x2-r5-nf1-w4", "1trip", 9, 20, 648, 64, False, True),
    Case("1t-fs-cw8x2-r5-nf1-w6", "1trip", 9, 20, 648, 96, False, True),
    Case("1t-fs-cw8x2-r5-nf1-w8", "1trip", 9, 20, 648, 128, False, True),
    Case("1t-fs-cw8x2-r5-nf2-w16", "1trip", 9, 20, 648, 512, False, True),
    Case("1t-fs-cw8x2-r5-nf3-w16", "1trip", 9, 20, 648, 768, False, True),
    Case("1t-fs-cw8x2-r5-nf4-w16", "1trip", 9, 20, 648, 1024, False, True),
    Case("1t-ln-cw2x2-r2-nf2-w16", "1trip", 1, 8, 8, 2048, True, False),
    Case("1t-ln-cw2x2-r2-nf3-w16", "1trip", 1, 8, 8, 3072, True, False),
    Case("1t-ln-cw2x2-r2-nf4-w16", "1trip", 1, 8, 8, 4096, True, False),
    Case("1t-ln-cw2x2-r5-nf2-w16", "1trip", 9, 20, 8, 2048, True, False),
    Case("1t-ln-cw2x2-r5-nf3-w16", "1trip", 9, 20, 8, 3072, True, False),
    Case("1t-ln-cw2x2-r5-nf4-w16", "1trip", 9, 20, 8, 4096, True, False),
    Case("1t-ln-cw4x2-r2-nf1-w2", "1trip", 1, 8, 8, 64, True, False),
    Case("1t-ln-cw4x2-r2-nf1-w3", "1trip", 1, 8, 8, 96, True, False),
    Case("1t-ln-cw4x2-r2-nf2-w10", "1trip", 1, 8, 8, 640, True, False),
    Case("1t-ln-cw4x2-r2-nf2-w11", "1trip", 1, 8, 8, 704, True, False),
    Case("1t-ln-cw4x2-r2-nf2-w12", "1trip", 1, 8, 8, 768, True, False),
    Case("1t-ln-cw4x2-r2-nf2-w13", "1trip", 1, 8, 8, 832, True, False),
    Case("1t-ln-cw4x2-r2-nf2-w14", "1trip", 1, 8, 8, 896, True, False),
    Case("1t-ln-cw4x2-r2-nf2-w15", "1trip", 1, 8, 8, 960, True, False),
    Case("1t-ln-cw4x2-r2-nf2-w2", "1trip", 1, 8, 8, 128, True, False),
    Case("1t-ln-cw4x2-r2-nf2-w3", "1trip", 1, 8, 8, 192, True, False),
    Case("1t-ln-cw4x2-r2-nf2-w4", "1trip", 1, 8, 8, 256, True, False),
    Case("1t-ln-cw4x2-r2-nf2-w5", "1trip", 1, 8, 8, 320, True, False),
    Case("1t-ln-cw4x2-r2-nf2-w6", "1trip", 1, 8, 8, 384, True, False),
    Case("1t-ln-cw4x2-r2-nf2-w7", "1trip", 1, 8, 8, 448, True, False),
    Case("1t-ln-cw4x2-r2-nf2-w8", "1trip", 1, 8, 8, 512, True, False),
    Case("1t-ln-cw4x2-r2-nf2-w9", "1trip", 1, 8, 8, 576, True, False),
    Case("1t-ln-cw4x2-r2-nf3-w16", "1trip", 1, 8, 8, 1536, True, False),
    Case("1t-ln-cw4x2-r2-nf4-w10", "1trip", 1, 8, 8, 1280, True, False),
    Case("1t-ln-cw4x2-r2-nf4-w11", "1trip", 1, 8, 8, 1408, True, False),
    Case("1t-ln-cw4x2-r2-nf4-w8", "1trip", 1, 8, 8, 1024, True, False),
    Case("1t-ln-cw4x2-r2-nf4-w9", "1trip", 1, 8, 8, 1152, True, False),
    Case("1t-ln-cw4x2-r5-nf1-w2", "1trip", 9, 20, 8, 64, True, False),
    Case("1t-ln-cw4x2-r5-nf1-w3", "1trip", 9, 20, 8, 96, True, False),
    Case("1t-ln-cw4x2-r5-nf2-w10", "1trip", 9, 20, 8, 640, True, False),
    Case("1t-ln-cw4x2-r5-nf2-w11", "1trip", 9, 20, 8, 704, True, False),
    Case("1t-ln-cw4x2-r5-nf2-w12", "1trip", 9, 20, 8, 768, True, False),
    Case("1t-ln-cw4x2-r5-nf2-w13", "1trip", 9, 20, 8, 832, True, False),
    Case("1t-ln-cw4x2-r5-nf2-w14", "1trip", 9, 20, 8, 896, True, False),
    Case("1t-ln-cw4x2-r5-nf2-w15", "1trip", 9, 20, 8, 960, True, False),
    Case("1t-ln-cw4x2-r5-nf2-w2", "1trip", 9, 20, 8, 128, True, False),
    Case("1t-ln-cw4x2-r5-nf2-w3", "1trip", 9, 20, 8, 192, True, False),
    Case("1t-ln-cw4x2-r5-nf2-w4", "1trip", 9, 20, 8, 256, True, False),
    Case("1t-ln-cw4x2-r5-nf2-w5", "1trip", 9, 20, 8, 320, True, False),
    Case("1t-ln-cw4x2-r5-nf2-w6", "1trip", 9, 20, 8, 384, True, False),
    Case("1t-ln-cw4x2-r5-nf2-w7", "1trip", 9, 20, 8, 448, True, False),
    Case("1t-ln-cw4x2-r5-nf2-w8", "1trip", 9, 20, 8, 512, True, False),
    Case("1t-ln-cw4x2-r5-nf2-w9", "1trip", 9, 20, 8, 576, True, False),
    Case("1t-ln-cw4x2-r5-nf3-w16", "1trip", 9, 20, 8, 1536, True, False),
    Case("1t-ln-cw4x2-r5-nf4-w10", "1trip", 9, 20, 8, 1280, True, False),
    Case("1t-ln-cw4x2-r5-nf4-w11", "1trip", 9, 20, 8, 1408, True, False),
    Case("1t-ln-cw4x2-r5-nf4-w8", "1trip", 9, 20, 8, 1024, True, False),
    Case("1t-ln-cw4x2-r5-nf4-w9", "1trip", 9, 20, 8, 1152, True, False),
    Case("1t-ln-cw8x2-r2-nf1-w12", "1trip", 1, 8, 648, 192, True, False),
    Case("1t-ln-cw8x2-r2-nf1-w16", "1trip", 1, 8, 648, 256, True, False),
    Case("1t-ln-cw8x2-r2-nf1-w4", "1trip", 1, 8, 648, 64, True, False),
    Case("1t-ln-cw8x2-r2-nf1-w6", "1trip", 1, 8, 648, 96, True, False),
    Case("1t-ln-cw8x2-r2-nf1-w8", "1trip", 1, 8, 648, 128, True, False),
    Case("1t-ln-cw8x2-r2-nf2-w16", "1trip", 1, 8, 648, 512, True, False),
    Case("1t-ln-cw8x2-r2-nf3-w16", "1trip", 1, 8, 648, 768, True, False),
    Case("1t-ln-cw8x2-r2-nf4-w16", "1trip", 1, 8, 648, 1024, True, False),
    Case("1t-ln-cw8x2-r5-nf1-w12", "1trip", 9, 20, 648, 192, True, False),
    Case("1t-ln-cw8x2-r5-nf1-w16", "1trip", 9, 20, 648, 256, True, False),
    Case("1t-ln-cw8x2-r5-nf1-w4", "1trip", 9, 20, 648, 64, True, False),
    Case("1t-ln-cw8x2-r5-nf1-w6", "1trip", 9, 20, 648, 96, True, False),
    Case("1t-ln-cw8x2-r5-nf1-w8", "1trip", 9, 20, 648, 128, True, False),
    Case("1t-ln-cw8x2-r5-nf2-w16", "1trip", 9, 20, 648, 512, True, False),
    Case("1t-ln-cw8x2-r5-nf3-w16", "1trip", 9, 20, 648, 768, True, False),
    Case("1t-ln-cw8x2-r5-nf4-w16", "1trip", 9, 20, 648, 1024, True, False),
    Case("1t-pl-cw2x2-r2-nf2-w16", "1trip", 1, 8, 8, 2048, False, False),
    Case("1t-pl-cw2x2-r2-nf3-w16", "1trip", 1, 8, 8, 3072, False, False),
    Case("1t-pl-cw2x2-r2-nf4-w16", "1trip", 1, 8, 8, 4096, False, False),
    Case("1t-pl-cw2x2-r5-nf2-w16", "1trip", 9, 20, 8, 2048, False, False),
    Case("1t-pl-cw2x2-r5-nf3-w16", "1trip", 9, 20, 8, 3072, False, False),
    Case("1t-pl-cw2x2-r5-nf4-w16", "1trip", 9, 20, 8, 4096, False, False),
    Case("1t-pl-cw4x2-r2-nf1-w2", "1trip", 1, 8, 8, 64, False, False),
    Case("1t-pl-cw4x2-r2-nf1-w3", "1trip", 1, 8, 8, 96, False, False),
    Case("1t-pl-cw4x2-r2-nf2-w10", "1trip", 1, 8, 8, 640, False, False),
    Case("1t-pl-cw4x2-r2-nf2-w11", "1trip", 1, 8, 8, 704, False, False),
    Case("1t-pl-cw4x2-r2-nf2-w12", "1trip", 1, 8, 8, 768, False, False),
    Case("1t-pl-cw4x2-r2-nf2-w13", "1trip", 1, 8, 8, 832, False, False),
    Case("1t-pl-cw4x2-r2-nf2-w14", "1trip", 1, 8, 8, 896, False, False),
    Case("1t-pl-cw4x2-r2-nf2-w15", "1trip", 1, 8, 8, 960, False, False),
    Case("1t-pl-cw4x2-r2-nf2-w2", "1trip", 1, 8, 8, 128, False, False),
    Case("1t-pl-cw4x2-r2-nf2-w3", "1trip", 1, 8, 8, 192, False, False),
    Case("1t-pl-cw4x2-r2-nf2-w4", "1trip", 1, 8, 8, 256, False, False),
    Case("1t-pl-cw4x2-r2-nf2-w5", "1trip", 1, 8, 8, 320, False, False),
    Case("1t-pl-cw4x2-r2-nf2-w6", "1trip", 1, 8, 8, 384, False, False),
    Case("1t-pl-cw4x2-r2-nf2-w7", "1trip", 1, 8, 8, 448, False, False),
    Case("1t-pl-cw4x2-r2-nf2-w8", "1trip", 1, 8, 8, 512, False, False),
    Case("1t-pl-cw4x2-r2-nf2-w9", "1trip", 1, 8, 8, 576, False, False),
    Case("1t-pl-cw4x2-r2-nf3-w16", "1trip", 1, 8, 8, 1536, False, False),
    Case("1t-pl-cw4x2-r2-nf4-w10", "1trip", 1, 8, 8, 1280, False, False),
    Case("1t-pl-cw4x2-r2-nf4-w11", "1trip", 1, 8, 8, 1408, False, False),
    Case("1t-pl-cw4x2-r2-nf4-w8", "1trip", 1, 8, 8, 1024, False, False),
    Case("1t-pl-cw4x2-r2-nf4-w9", "1trip", 1, 8, 8, 1152, False, False),
    Case("1t-pl-cw4x2-r5-nf1-w2", "1trip", 9, 20, 8, 64, False, False),
    Case("1t-pl-cw4x2-r5-nf1-w3", "1trip", 9, 20, 8, 96, False, False),
    Case("1t-pl-cw4x2-r5-nf2-w10", "1trip", 9, 20, 8, 640, False, False),
    Case("1t-pl-cw4x2-r5-nf2-w11", "1trip", 9, 20, 8, 704, False, False),
    Case("1t-pl-cw4x2-r5-nf2-w12", "1trip", 9, 20, 8, 768, False, False),
    Case("1t-pl-cw4x2-r5-nf2-w13", "1trip", 9, 20, 8, 832, False, False),
    Case("1t-pl-cw4x2-r5-nf2-w14", "1trip", 9, 20, 8, 896, False, False),
    Case("1t-pl-cw4x2-r5-nf2-w15", "1trip", 9, 20, 8, 960, False, False),
    Case("1t-pl-cw4x2-r5-nf2-w2", "1trip", 9, 20, 8, 128, False, False),
    Case("1t-pl-cw4x2-r5-nf2-w3", "1trip", 9, 20, 8, 192, False, False),
    Case("1t-pl-cw4x2-r5-nf2-w4", "1trip", 9, 20, 8, 256, False, False),
    Case("1t-pl-cw4x2-r5-nf2-w5", "1trip", 9, 20, 8, 320, False, False),
    Case("1t-pl-cw4x2-r5-nf2-w6", "1trip", 9, 20, 8, 384, False, False),
    Case("1t-pl-cw4x2-r5-nf2-w7", "1trip", 9, 20, 8, 448, False, False),
    Case("1t-pl-cw4x2-r5-nf2-w8", "1trip", 9, 20, 8, 512, False, False),
    Case("1t-pl-cw4x2-r5-nf2-w9", "1trip", 9, 20, 8, 576, False, False),
    Case("1t-pl-cw4x2-r5-nf3-w16", "1trip", 9, 20, 8, 1536, False, False),
    Case("1t-pl-cw4x2-r5-nf4-w10", "1trip", 9, 20, 8, 1280, False, False),
    Case("1t-pl-cw4x2-r5-nf4-w11", "1trip", 9, 20, 8, 1408, False, False),
    Case("1t-pl-cw4x2-r5-nf4-w8", "1trip", 9, 20, 8, 1024, False, False),
    Case("1t-pl-cw4x2-r5-nf4-w9", "1trip", 9, 20, 8, 1152, False, False),
    Case("1t-pl-cw8x2-r2-nf1-w12", "1trip", 1, 8, 648, 192, False, False),
    Case("1t-pl-cw8x2-r2-nf1-w16", "1trip", 1, 8, 648, 256, False, False),
    Case("1t-pl-cw8x2-r2-nf1-w4", "1trip", 1, 8, 648, 64, False, False),
    Case("1t-pl-cw8x2-r2-nf1-w6", "1trip", 1, 8, 648, 96, False, False),
    Case("1t-pl-cw8x2-r2-nf1-w8", "1trip", 1, 8, 648, 128, False, False),
    Case("1t-pl-cw8x2-r2-nf2-w16", "1trip", 1, 8, 648, 512, False, False),
    Case("1t-pl-cw8x2-r2-nf3-w16", "1trip", 1, 8, 648, 768, False, False),
    Case("1t-pl-cw8x2-r2-nf4-w16", "1trip", 1, 8, 648, 1024, False, False),
    Case("1t-pl-cw8x2-r5-nf1-w12", "1trip", 9, 20, 648, 192, False, False),
    Case("1t-pl-cw8x2-r5-nf1-w16", "1trip", 9, 20, 648, 256, False, False),
    Case("1t-pl-cw8x2-r5-nf1-w4", "1trip", 9, 20, 648, 64, False, False),
    Case("1t-pl-cw8x2-r5-nf1-w6", "1trip", 9, 20, 648, 96, False, False),
    Case("1t-pl-cw8x2-r5-nf1-w8", "1trip", 9, 20, 648, 128, False, False),
    Case("1t-pl-cw8x2-r5-nf2-w16", "1trip", 9, 20, 648, 512, False, False),
    Case("1t-pl-cw8x2-r5-nf3-w16", "1trip", 9, 20, 648, 768, False, False),
    Case("1t-pl-cw8x2-r5-nf4-w16", "1trip", 9, 20, 648, 1024, False, False),
    Case("mat-ln-cw32-k1", "ln_gemm", 1, 32, 4100, 128, True, False),
    Case("mat-ln-cw32-k1r", "ln_gemm", 1, 32, 4100, 64, True, False),
    Case("mat-ln-cw32-k4", "ln_gemm", 1, 32, 4100, 512, True, False),
    Case("mat-ln-cw32-k4r", "ln_gemm", 1, 32, 4100, 448, True, False),
    Case("mat-ln-cw32-k5", "ln_gemm", 1, 32, 4100, 640, True, False),
    Case("mat-ln-cw32-k5r", "ln_gemm", 1, 32, 4100, 544, True, False),
    Case("mat-ln-cw4-k1r", "ln_gemm", 1, 32, 7, 96, True, False),
    Case("mat-ln-cw4-k5r", "ln_gemm", 1, 32, 7, 544, True, False),
    Case("mat-ln-cw8-k1r", "ln_gemm", 1, 32, 644, 96, True, False),
    Case("mat-ln-cw8-k5r", "ln_gemm", 1, 32, 644, 544, True, False),
    Case("mat-pl-cw32-k1", "ln_gemm", 1, 32, 4100, 128, False, False),
    Case("mat-pl-cw32-k1r", "ln_gemm", 1, 32, 4100, 64, False, False),
    Case("mat-pl-cw32-k4", "ln_gemm", 1, 32, 4100, 512, False, False),
    Case("mat-pl-cw32-k4r", "ln_gemm", 1, 32, 4100, 448, False, False),
    Case("mat-pl-cw32-k5", "ln_gemm", 1, 32, 4100, 640, False, False),
    Case("mat-pl-cw32-k5r", "ln_gemm", 1, 32, 4100, 544, False, False),
    Case("mat-pl-cw4-k1r", "ln_gemm", 1, 32, 7, 96, False, False),
    Case("mat-pl-cw4-k5r", "ln_gemm", 1, 32, 7, 544, False, False),
    Case("mat-pl-cw8-k1r", "ln_gemm", 1, 32, 644, 96, False, False),
    Case("mat-pl-cw8-k5r", "ln_gemm", 1, 32, 644, 544, False, False),
    Case("vec-ln-cw2-mr16-w16-k1", "ln_gemm", 9, 16, 7, 2048, True, False),
    Case("vec-ln-cw2-mr16-w16-k1r", "ln_gemm", 9, 16, 7, 1024, True, False),
    Case("vec-ln-cw2-mr24-w16-k1", "ln_gemm", 17, 24, 7, 2048, True, False),
    Case("vec-ln-cw2-mr24-w16-k1r", "ln_gemm", 17, 24, 7, 1024, True, False),
    Case("vec-ln-cw2-mr32-w16-k1", "ln_gemm", 25, 32, 7, 2048, True, False),
    Case("vec-ln-cw2-mr32-w16-k1r", "ln_gemm", 25, 32, 7, 1024, True, False),
    Case("vec-ln-cw2-mr8-w16-k1", "ln_gemm", 1, 8, 7, 2048, True, False),
    Case("vec-ln-cw2-mr8-w16-k1r", "ln_gemm", 1, 8, 7, 1024, True, False),
    Case("vec-ln-cw4-mr16-w16-k1r", "ln_gemm", 9, 16, 7, 64, True, False),
    Case("vec-ln-cw4-mr16-w16-k2r", "ln_gemm", 9, 16, 7, 1088, True, False),
    Case("vec-ln-cw4-mr24-w16-k1r", "ln_gemm", 17, 24, 7, 64, True, False),
    Case("vec-ln-cw4-mr24-w16-k2r", "ln_gemm", 17, 24, 7, 1088, True, False),
    Case("vec-ln-cw4-mr32-w16-k1r", "ln_gemm", 25, 32, 7, 64, True, False),
    Case("vec-ln-cw4-mr32-w16-k2r", "ln_gemm", 25, 32, 7, 1088, True, False),
    Case("vec-ln-cw4-mr8-w16-k1r", "ln_gemm", 1, 8, 7, 64, True, False),
    Case("vec-ln-cw4-mr8-w16-k2r", "ln_gemm", 1, 8, 7, 1088, True, False),
    Case("vec-ln-cw8-mr16-w16-k1", "ln_gemm", 9, 16, 644, 512, True, False),
    Case("vec-ln-cw8-mr16-w16-k1r", "ln_gemm", 9, 16, 644, 64, True, False),
    Case("vec-ln-cw8-mr16-w16-k2", "ln_gemm", 9, 16, 644, 1024, True, False),
    Case("vec-ln-cw8-mr16-w16-k2r", "ln_gemm", 9, 16, 644, 576, True, False),
    Case("vec-ln-cw8-mr16-w16-k3", "ln_gemm", 9, 16, 644, 1536, True, False),
    Case("vec-ln-cw8-mr16-w16-k3r", "ln_gemm", 9, 16, 644, 1088, True, False),
    Case("vec-ln-cw8-mr24-w16-k1", "ln_gemm", 17, 24, 644, 512, True, False),
    Case("vec-ln-cw8-mr24-w16-k1r", "ln_gemm", 17, 24, 644, 64, True, False),
    Case("vec-ln-cw8-mr24-w16-k2", "ln_gemm", 17, 24, 644, 1024, True, False),
    Case("vec-ln-cw8-mr24-w16-k2r", "ln_gemm", 17, 24, 644, 576, True, False),
    Case("vec-ln-cw8-mr24-w16-k3", "ln_gemm", 17, 24, 644, 1536, True, False),
    Case("vec-ln-cw8-mr24-w16-k3r", "ln_gemm", 17, 24, 644, 1088, True, False),
    Case("vec-ln-cw8-mr32-w16-k1", "ln_gemm", 25, 32, 644, 512, True, False),
    Case("vec-ln-cw8-mr32-w16-k1r", "ln_gemm", 25, 32, 644, 64, True, False),
    Case("vec-ln-cw8-mr32-w16-k2", "ln_gemm", 25, 32, 644, 1024, True, False),
    Case("vec-ln-cw8-mr32-w16-k2r", "ln_gemm", 25, 32, 644, 576, True, False),
    Case("vec-ln-cw8-mr32-w16-k3", "ln_gemm", 25, 32, 644, 1536, True, False),
    Case("vec-ln-cw8-mr32-w16-k3r", "ln_gemm", 25, 32, 644, 1088, True, False),
    Case("vec-ln-cw8-mr8-w16-k1", "ln_gemm", 1, 8, 644, 512, True, False),
    Case("vec-ln-cw8-mr8-w16-k1r", "ln_gemm", 1, 8, 644, 64, True, False),
    Case("vec-ln-cw8-mr8-w16-k2", "ln_gemm", 1, 8, 644, 1024, True, False),
    Case("vec-ln-cw8-mr8-w16-k2r", "ln_gemm", 1, 8, 644, 576, True, False),
    Case("vec-ln-cw8-mr8-w16-k3", "ln_gemm", 1, 8, 644, 1536, True, False),
    Case("vec-ln-cw8-mr8-w16-k3r", "ln_gemm", 1, 8, 644, 1088, True, False),
    Case("vec-pl-cw2-mr16-w10-k1", "ln_gemm", 9, 16, 7, 1280, False, False),
    Case("vec-pl-cw2-mr16-w11-k1", "ln_gemm", 9, 16, 7, 1408, False, False),
    Case("vec-pl-cw2-mr16-w12-k1", "ln_gemm", 9, 16, 7, 1536, False, False),
    Case("vec-pl-cw2-mr16-w13-k1", "ln_gemm", 9, 16, 7, 1664, False, False),
    Case("vec-pl-cw2-mr16-w14-k1", "ln_gemm", 9, 16, 7, 1792, False, False),
    Case("vec-pl-cw2-mr16-w15-k1", "ln_gemm", 9, 16, 7, 1920, False, False),
    Case("vec-pl-cw2-mr16-w16-k1", "ln_gemm", 9, 16, 7, 2048, False, False),
    Case("vec-pl-cw2-mr16-w16-k2", "ln_gemm", 9, 16, 7, 4096, False, False),
    Case("vec-pl-cw2-mr16-w16-k2r", "ln_gemm", 9, 16, 7, 2176, False, False),
    Case("vec-pl-cw2-mr16-w8-k1", "ln_gemm", 9, 16, 7, 1024, False, False),
    Case("vec-pl-cw2-mr16-w9-k1", "ln_gemm", 9, 16, 7, 1152, False, False),
    Case("vec-pl-cw2-mr24-w10-k1", "ln_gemm", 17, 24, 7, 1280, False, False),
    Case("vec-pl-cw2-mr24-w11-k1", "ln_gemm", 17, 24, 7, 1408, False, False),
    Case("vec-pl-cw2-mr24-w12-k1", "ln_gemm", 17, 24, 7, 1536, False, False),
    Case("vec-pl-cw2-mr24-w13-k1", "ln_gemm", 17, 24, 7, 1664, False, False),
    Case("vec-pl-cw2-mr24-w14-k1", "ln_gemm", 17, 24, 7, 1792, False, False),
    Case("vec-pl-cw2-mr24-w15-k1", "ln_gemm", 17, 24, 7, 1920, False, False),
    Case("vec-pl-cw2-mr24-w16-k1", "ln_gemm", 17, 24, 7, 2048, False, False),
    Case("vec-pl-cw2-mr24-w16-k2", "ln_gemm", 17, 24, 7, 4096, False, False),
    Case("vec-pl-cw2-mr24-w16-k2r", "ln_gemm", 17, 24, 7, 2176, False, False),
    Case("vec-pl-cw2-mr24-w8-k1", "ln_gemm", 17, 24, 7, 1024, False, False),
    Case("vec-pl-cw2-mr24-w9-k1", "ln_gemm", 17, 24, 7, 1152, False, False),
    Case("vec-pl-cw2-mr32-w10-k1", "ln_gemm", 25, 32, 7, 1280, False, False),
    Case("vec-pl-cw2-mr32-w11-k1", "ln_gemm", 25, 32, 7, 1408, False, False),
    Case("vec-pl-cw2-mr32-w12-k1", "ln_gemm", 25, 32, 7, 1536, False, False),
    Case("vec-pl-cw2-mr32-w13-k1", "ln_gemm", 25, 32, 7, 1664, False, False),
    Case("vec-pl-cw2-mr32-w14-k1", "ln_gemm", 25, 32, 7, 1792, False, False),
    Case("vec-pl-cw2-mr32-w15-k1", "ln_gemm", 25, 32, 7, 1920, False, False),
    Case("vec-pl-cw2-mr32-w16-k1", "ln_gemm", 25, 32, 7, 2048, False, False),
    Case("vec-pl-cw2-mr32-w16-k2", "ln_gemm", 25, 32, 7, 4096, False, False),
    Case("vec-pl-cw2-mr32-w16-k2r", "ln_gemm", 25, 32, 7, 2176, False, False),
    Case("vec-pl-cw2-mr32-w8-k1", "ln_gemm", 25, 32, 7, 1024, False, False),
    Case("vec-pl-cw2-mr32-w9-k1", "ln_gemm", 25, 32, 7, 1152, False, False),
    Case("vec-pl-cw2-mr8-w10-k1", "ln_gemm", 1, 8, 7, 1280, False, False),
    Case("vec-pl-cw2-mr8-w11-k1", "ln_gemm", 1, 8, 7, 1408, False, False),
    Case("vec-pl-cw2-mr8-w12-k1", "ln_gemm", 1, 8, 7, 1536, False, False),
    Case("vec-pl-cw2-mr8-w13-k1", "ln_gemm", 1, 8, 7, 1664, False, False),
    Case("vec-pl-cw2-mr8-w14-k1", "ln_gemm", 1, 8, 7, 1792, False, False),
    Case("vec-pl-cw2-mr8-w15-k1", "ln_gemm", 1, 8, 7, 1920, False, False),
    Case("vec-pl-cw2-mr8-w16-k1", "ln_gemm", 1, 8, 7, 2048, False, False),
    Case("vec-pl-cw2-mr8-w16-k2", "ln_gemm", 1, 8, 7, 4096, False, False),
    Case("vec-pl-cw2-mr8-w16-k2r", "ln_gemm", 1, 8, 7, 2176, False, False),
    Case("vec-pl-cw2-mr8-w8-k1", "ln_gemm", 1, 8, 7, 1024, False, False),
    Case("vec-pl-cw2-mr8-w9-k1", "ln_gemm", 1, 8, 7, 1152, False, False),
    Case("vec-pl-cw4-mr16-w1-k1", "ln_gemm", 9, 16, 7, 64, False, False),
    Case("vec-pl-cw4-mr16-w10-k1", "ln_gemm", 9, 16, 7, 640, False, False),
    Case("vec-pl-cw4-mr16-w11-k1", "ln_gemm", 9, 16, 7, 704, False, False),
    Case("vec-pl-cw4-mr16-w12-k1", "ln_gemm", 9, 16, 7, 768, False, False),
    Case("vec-pl-cw4-mr16-w13-k1", "ln_gemm", 9, 16, 7, 832, False, False),
    Case("vec-pl-cw4-mr16-w14-k1", "ln_gemm", 9, 16, 7, 896, False, False),
    Case("vec-pl-cw4-mr16-w15-k1", "ln_gemm", 9, 16, 7, 960, False, False),
    Case("vec-pl-cw4-mr16-w16-k2r", "ln_gemm", 9, 16, 7, 1088, False, False),
    Case("vec-pl-cw4-mr16-w16-k3r", "ln_gemm", 9, 16, 7, 2112, False, False),
    Case("vec-pl-cw4-mr16-w2-k1", "ln_gemm", 9, 16, 7, 128, False, False),
    Case("vec-pl-cw4-mr16-w3-k1", "ln_gemm", 9, 16, 7, 192, False, False),
    Case("vec-pl-cw4-mr16-w4-k1", "ln_gemm", 9, 16, 7, 256, False, False),
    Case("vec-pl-cw4-mr16-w5-k1", "ln_gemm", 9, 16, 7, 320, False, False),
    Case("vec-pl-cw4-mr16-w6-k1", "ln_gemm", 9, 16, 7, 384, False, False),
    Case("vec-pl-cw4-mr16-w7-k1", "ln_gemm", 9, 16, 7, 448, False, False),
    Case("vec-pl-cw4-mr16-w8-k1", "ln_gemm", 9, 16, 7, 512, False, False),
    Case("vec-pl-cw4-mr16-w9-k1", "ln_gemm", 9, 16, 7, 576, False, False),
    Case("vec-pl-cw4-mr24-w10-k1", "ln_gemm", 17, 24, 7, 640, False, False),
    Case("vec-pl-cw4-mr24-w11-k1", "ln_gemm", 17, 24, 7, 704, False, False),
    Case("vec-pl-cw4-mr24-w12-k1", "ln_gemm", 17, 24, 7, 768, False, False),
    Case("vec-pl-cw4-mr24-w13-k1", "ln_gemm", 17, 24, 7, 832, False, False),
    Case("vec-pl-cw4-mr24-w14-k1", "ln_gemm", 17, 24, 7, 896, False, False),
    Case("vec-pl-cw4-mr24-w15-k1", "ln_gemm", 17, 24, 7, 960, False, False),
    Case("vec-pl-cw4-mr24-w16-k2r", "ln_gemm", 17, 24, 7, 1088, False, False),
    Case("vec-pl-cw4-mr24-w16-k3r", "ln_gemm", 17, 24, 7, 2112, False, False),
    Case("vec-pl-cw4-mr24-w2-k1", "ln_gemm", 17, 24, 7, 128, False, False),
    Case("vec-pl-cw4-mr24-w2-k1r", "ln_gemm", 17, 24, 7, 64, False, False),
    Case("vec-pl-cw4-mr24-w3-k1", "ln_gemm", 17, 24, 7, 192, False, False),
    Case("vec-pl-cw4-mr24-w4-k1", "ln_gemm", 17, 24, 7, 256, False, False),
    Case("vec-pl-cw4-mr24-w5-k1", "ln_gemm", 17, 24, 7, 320, False, False),
    Case("vec-pl-cw4-mr24-w6-k1", "ln_gemm", 17, 24, 7, 384, False, False),
    Case("vec-pl-cw4-mr24-w7-k1", "ln_gemm", 17, 24, 7, 448, False, False),
    Case("vec-pl-cw4-mr24-w8-k1", "ln_gemm", 17, 24, 7, 512, False, False),
    Case("vec-pl-cw4-mr24-w9-k1", "ln_gemm", 17, 24, 7, 576, False, False),
    Case("vec-pl-cw4-mr32-w10-k1", "ln_gemm", 25, 32, 7, 640, False, False),
    Case("vec-pl-cw4-mr32-w11-k1", "ln_gemm", 25, 32, 7, 704, False, False),
    Case("vec-pl-cw4-mr32-w12-k1", "ln_gemm", 25, 32, 7, 768, False, False),
    Case("vec-pl-cw4-mr32-w13-k1", "ln_gemm", 25, 32, 7, 832, False, False),
    Case("vec-pl-cw4-mr32-w14-k1", "ln_gemm", 25, 32, 7, 896, False, False),
    Case("vec-pl-cw4-mr32-w15-k1", "ln_gemm", 25, 32, 7, 960, False, False),
    Case("vec-pl-cw4-mr32-w16-k2r", "ln_gemm", 25, 32, 7, 1088, False, False),
    Case("vec-pl-cw4-mr32-w16-k3r", "ln_gemm", 25, 32, 7, 2112, False, False),
    Case("vec-pl-cw4-mr32-w2-k1", "ln_gemm", 25, 32, 7, 128, False, False),
    Case("vec-pl-cw4-mr32-w2-k1r", "ln_gemm", 25, 32, 7, 64, False, False),
    Case("vec-pl-cw4-mr32-w3-k1", "ln_gemm", 25, 32, 7, 192, False, False),
    Case("vec-pl-cw4-mr32-w4-k1", "ln_gemm", 25, 32, 7, 256, False, False),
    Case("vec-pl-cw4-mr32-w5-k1", "ln_gemm", 25, 32, 7, 320, False, False),
    Case("vec-pl-cw4-mr32-w6-k1", "ln_gemm", 25, 32, 7, 384, False, False),
    Case("vec-pl-cw4-mr32-w7-k1", "ln_gemm", 25, 32, 7, 448, False, False),
    Case("vec-pl-cw4-mr32-w8-k1", "ln_gemm", 25, 32, 7, 512, False, False),
    Case("vec-pl-cw4-mr32-w9-k1", "ln_gemm", 25, 32, 7, 576, False, False),
    Case("vec-pl-cw4-mr8-w1-k1", "ln_gemm", 1, 8, 7, 64, False, False),
    Case("vec-pl-cw4-mr8-w10-k1", "ln_gemm", 1, 8, 7, 640, False, False),
    Case("vec-pl-cw4-mr8-w11-k1", "ln_gemm", 1, 8, 7, 704, False, False),
    Case("vec-pl-cw4-mr8-w12-k1", "ln_gemm", 1, 8, 7, 768, False, False),
    Case("vec-pl-cw4-mr8-w13-k1", "ln_gemm", 1, 8, 7, 832, False, False),
    Case("vec-pl-cw4-mr8-w14-k1", "ln_gemm", 1, 8, 7, 896, False, False),
    Case("vec-pl-cw4-mr8-w15-k1", "ln_gemm", 1, 8, 7, 960, False, False),
    Case("vec-pl-cw4-mr8-w16-k2r", "ln_gemm", 1, 8, 7, 1088, False, False),
    Case("vec-pl-cw4-mr8-w16-k3r", "ln_gemm", 1, 8, 7, 2112, False, False),
    Case("vec-pl-cw4-mr8-w2-k1", "ln_gemm", 1, 8, 7, 128, False, False),
    Case("vec-pl-cw4-mr8-w3-k1", "ln_gemm", 1, 8, 7, 192, False, False),
    Case("vec-pl-cw4-mr8-w4-k1", "ln_gemm", 1, 8, 7, 256, False, False),
    Case("vec-pl-cw4-mr8-w5-k1", "ln_gemm", 1, 8, 7, 320, False, False),
    Case("vec-pl-cw4-mr8-w6-k1", "ln_gemm", 1, 8, 7, 384, False, False),
    Case("vec-pl-cw4-mr8-w7-k1", "ln_gemm", 1, 8, 7, 448, False, False),
    Case("vec-pl-cw4-mr8-w8-k1", "ln_gemm", 1, 8, 7, 512, False, False),
    Case("vec-pl-cw4-mr8-w9-k1", "ln_gemm", 1, 8, 7, 576, False, False),
    Case("vec-pl-cw8-mr16-w10-k1", "ln_gemm", 9, 16, 644, 320, False, False),
    Case("vec-pl-cw8-mr16-w12-k1", "ln_gemm", 9, 16, 644, 384, False, False),
    Case("vec-pl-cw8-mr16-w14-k1", "ln_gemm", 9, 16, 644, 448, False, False),
    Case("vec-pl-cw8-mr16-w16-k1", "ln_gemm", 9, 16, 644, 512, False, False),
    Case("vec-pl-cw8-mr16-w16-k2", "ln_gemm", 9, 16, 644, 1024, False, False),
    Case("vec-pl-cw8-mr16-w16-k2r", "ln_gemm", 9, 16, 644, 576, False, False),
    Case("vec-pl-cw8-mr16-w16-k3", "ln_gemm", 9, 16, 644, 1536, False, False),
    Case("vec-pl-cw8-mr16-w16-k3r", "ln_gemm", 9, 16, 644, 1088, False, False),
    Case("vec-pl-cw8-mr16-w2-k1", "ln_gemm", 9, 16, 644, 64, False, False),
    Case("vec-pl-cw8-mr16-w4-k1", "ln_gemm", 9, 16, 644, 128, False, False),
    Case("vec-pl-cw8-mr16-w6-k1", "ln_gemm", 9, 16, 644, 192, False, False),
    Case("vec-pl-cw8-mr16-w8-k1", "ln_gemm", 9, 16, 644, 256, False, False),
    Case("vec-pl-cw8-mr24-w10-k1", "ln_gemm", 17, 24, 644, 320, False, False),
    Case("vec-pl-cw8-mr24-w12-k1", "ln_gemm", 17, 24, 644, 384, False, False),
    Case("vec-pl-cw8-mr24-w14-k1", "ln_gemm", 17, 24, 644, 448, False, False),
    Case("vec-pl-cw8-mr24-w16-k1", "ln_gemm", 17, 24, 644, 512, False, False),
    Case("vec-pl-cw8-mr24-w16-k2", "ln_gemm", 17, 24, 644, 1024, False, False),
    Case("vec-pl-cw8-mr24-w16-k2r", "ln_gemm", 17, 24, 644, 576, False, False),
    Case("vec-pl-cw8-mr24-w16-k3", "ln_gemm", 17, 24, 644, 1536, False, False),
    Case("vec-pl-cw8-mr24-w16-k3r", "ln_gemm", 17, 24, 644, 1088, False, False),
    Case("vec-pl-cw8-mr24-w3-k1r", "ln_gemm", 17, 24, 644, 64, False, False),
    Case("vec-pl-cw8-mr24-w4-k1", "ln_gemm", 17, 24, 644, 128, False, False),
    Case("vec-pl-cw8-mr24-w6-k1", "ln_gemm", 17, 24, 644, 192, False, False),
    Case("vec-pl-cw8-mr24-w8-k1", "ln_gemm", 17, 24, 644, 256, False, False),
    Case("vec-pl-cw8-mr32-w10-k1", "ln_gemm", 25, 32, 644, 320, False, False),
    Case("vec-pl-cw8-mr32-w12-k1", "ln_gemm", 25, 32, 644, 384, False, False),
    Case("vec-pl-cw8-mr32-w14-k1", "ln_gemm", 25, 32, 644, 448, False, False),
    Case("vec-pl-cw8-mr32-w16-k1", "ln_gemm", 25, 32, 644, 512, False, False),
    Case("vec-pl-cw8-mr32-w16-k2", "ln_gemm", 25, 32, 644, 1024, False, False),
    Case("vec-pl-cw8-mr32-w16-k2r", "ln_gemm", 25, 32, 644, 576, False, False),
    Case("vec-pl-cw8-mr32-w16-k3", "ln_gemm", 25, 32, 644, 1536, False, False),
    Case("vec-pl-cw8-mr32-w16-k3r", "ln_gemm", 25, 32, 644, 1088, False, False),
    Case("vec-pl-cw8-mr32-w4-k1", "ln_gemm", 25, 32, 644, 128, False, False),
    Case("vec-pl-cw8-mr32-w4-k1r", "ln_gemm", 25, 32, 644, 64, False, False),
    Case("vec-pl-cw8-mr32-w6-k1", "ln_gemm", 25, 32, 644, 192, False, False),
    Case("vec-pl-cw8-mr32-w8-k1", "ln_gemm", 25, 32, 644, 256, False, False),
    Case("vec-pl-cw8-mr8-w10-k1", "ln_gemm", 1, 8, 644, 320, False, False),
    Case("vec-pl-cw8-mr8-w12-k1", "ln_gemm", 1, 8, 644, 384, False, False),
    Case("vec-pl-cw8-mr8-w14-k1", "ln_gemm", 1, 8, 644, 448, False, False),
    Case("vec-pl-cw8-mr8-w16-k1", "ln_gemm", 1, 8, 644, 512, False, False),
    Case("vec-pl-cw8-mr8-w16-k2", "ln_gemm", 1, 8, 644, 1024, False, False),
    Case("vec-pl-cw8-mr8-w16-k2r", "ln_gemm", 1, 8, 644, 576, False, False),
    Case("vec-pl-cw8-mr8-w16-k3", "ln_gemm", 1, 8, 644, 1536, False, False),
    Case("vec-pl-cw8-mr8-w16-k3r", "ln_gemm", 1, 8, 644, 1088, False, False),
    Case("vec-pl-cw8-mr8-w2-k1", "ln_gemm", 1, 8, 644, 64, False, False),
    Case("vec-pl-cw8-mr8-w4-k1", "ln_gemm", 1, 8, 644, 128, False, False),
    Case("vec-pl-cw8-mr8-w6-k1", "ln_gemm", 1, 8, 644, 192, False, False),
    Case("vec-pl-cw8-mr8-w8-k1", "ln_gemm", 1, 8, 644, 256, False, False),
]

CASES = PINNED + REPRESENTATIVES


if __name__ == "__main__":
    import importlib
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as ge
    ge.load_package()
    _ops = importlib.import_module("asr_2pass_amd.ops")
    print("REPRESENTATIVES = [")
    for c in representatives(_ops):
        print(f'    Case("{c.route}", "{c.form}", {c.m_lo}, {c.m_hi}, {c.N}, {c.K}, {c.ln}, {c.fsmn}),')
    print("]")
