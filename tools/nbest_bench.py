#!/usr/bin/env python3
"""What the N-best head costs ("N-best candidates and token confidence").

  head   launch time of the head at the headline shape (7,015 rows x 8,404 columns, ld 8,448), HIP events around back-to-back
         launches: the arg-max kernel ids-only and with logp, the top-k kernel at k = 1, 5, 8 with logp null; the variants
         alternate inside every round, the median over the rounds is printed
  host   wall time of pfhip_offline_forward with logp against pfhip_offline_forward_nbest(k = 5) without, on the headline batch
         (32 x 30 s, synthetic Paraformer-large), output buffers allocated and touched once outside the timed calls

  python tools/nbest_bench.py [head|host|all] [--rounds 7] [--launches 50]
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def head_times(ops, torch, rounds, launches, rows=7015, V=8404, ld=8448):
    g = torch.Generator(device="cuda").manual_seed(5)
    x = 4.0 * torch.randn((rows, ld), generator=g, device="cuda", dtype=torch.float32)
    lib, p, st = ops._lib(), ops._p, ops._stream
    logp = torch.empty((rows, V), dtype=torch.float32, device="cuda")
    ids = torch.empty(rows, dtype=torch.int32, device="cuda")
    tk_ids = torch.empty((rows, 8), dtype=torch.int32, device="cuda")
    tk_logp = torch.empty((rows, 8), dtype=torch.float32, device="cuda")
    variants = {
        "argmax, ids only": lambda: lib.pfhip_op_logsoftmax_argmax(p(x), ld, rows, V, None, p(ids), st()),
        "argmax, logp written": lambda: lib.pfhip_op_logsoftmax_argmax(p(x), ld, rows, V, p(logp), p(ids), st()),
    }
    for k in (1, 5, 8):
        variants[f"topk k={k}, no logp"] = (lambda k=k: lib.pfhip_op_logsoftmax_topk(p(x), ld, rows, V, k, None, p(ids), p(tk_ids),
                                                                                    p(tk_logp), st()))
    variants["topk k=5, logp written"] = lambda: lib.pfhip_op_logsoftmax_topk(p(x), ld, rows, V, 5, p(logp), p(ids), p(tk_ids), p(tk_logp), st())
    for fn in variants.values():
        for _ in range(5):
            assert fn() == 0
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / launches)
    out = {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for name, v in ms.items()}
    out["ratio topk k=5 no logp / argmax logp written"] = out["topk k=5, no logp"]["median_ms"] / out["argmax, logp written"]["median_ms"]
    out["shape"] = f"{rows} rows x {V} columns, ld {ld}; {launches} launches per window, {rounds} rounds"
    return out


def host_times(pkg, rounds, batch=32, seconds=30):
    weights = importlib.import_module("asr_2pass_amd.weights")
    man, blob = weights.synth_weights(dict(weights.PARAFORMER_LARGE), seed=1234)
    model = pkg.ParaformerHip().InitAsr((man, blob))
    lib, h, V = model._lib, model._h, model.vocab_size
    rng = np.random.default_rng(20251114)
    n = seconds * 16000
    t = np.arange(n) / 16000.0
    utts = [np.clip(np.round(8000 * (0.6 * np.sin(2 * np.pi * (110.0 * 2.0 ** ((i % 24) / 12.0)) * t) + 0.4 * rng.standard_normal(n))),
                    -32768, 32767).astype(np.float32) / 32768.0 for i in range(batch)]
    mt = n // 960 + 2
    lens = (ctypes.c_int * batch)(*[n] * batch)
    ptrs = (ctypes.c_void_p * batch)(*[u.ctypes.data for u in utts])
    ids = np.zeros((batch, mt), np.int32)
    tn, nf = np.zeros(batch, np.int32), np.zeros(batch, np.int32)
    logp = np.ones((batch, mt, V), np.float32)          # touched: no page faults inside the timed calls
    nb_ids, nb_logp = np.ones((batch, mt, 5), np.int32), np.ones((batch, mt, 5), np.float32)
    i32, f32 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)

    def out_struct(with_logp):
        o = pkg._Out()
        o.token_ids, o.token_num, o.n_fires = ids.ctypes.data_as(i32), tn.ctypes.data_as(i32), nf.ctypes.data_as(i32)
        o.logp = logp.ctypes.data_as(f32) if with_logp else None
        o.max_tokens = mt
        return o
    o_logp, o_ids = out_struct(True), out_struct(False)
    nb = pkg._Nbest(5, nb_ids.ctypes.data_as(i32), nb_logp.ctypes.data_as(f32))
    sof = (ctypes.c_int * batch)(*[0] * batch)
    calls = {
        "forward, ids only": lambda: lib.pfhip_offline_forward(h, ptrs, lens, batch, None, 0, ctypes.byref(o_ids)),
        "forward, logp": lambda: lib.pfhip_offline_forward(h, ptrs, lens, batch, None, 0, ctypes.byref(o_logp)),
        "forward_nbest k=5, no logp": lambda: lib.pfhip_offline_forward_nbest(h, ptrs, lens, batch, None, None, 0, sof, ctypes.byref(o_ids),
                                                                              ctypes.byref(nb)),
    }
    for fn in calls.values():
        for _ in range(2):
            assert fn() == 0
    ms = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            assert fn() == 0                              # ends in the forward's own synchronise: the results are on the host
            ms[name].append(1e3 * (time.perf_counter() - t0))
    out = {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for name, v in ms.items()}
    rows = int(nf.sum())
    out["token_rows"] = rows
    out["bytes_logp"] = rows * V * 4
    out["bytes_nbest_k5"] = rows * 5 * 8
    model.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=["head", "host", "all"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("nbest_bench.py needs a GPU (no CPU path)")
    import __graft_entry__ as ge
    pkg = ge.load_package()
    res = {}
    if args.what in ("head", "all"):
        res["head"] = head_times(importlib.import_module("asr_2pass_amd.ops"), torch, args.rounds, args.launches)
    if args.what in ("host", "all"):
        res["host"] = host_times(pkg, args.rounds)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
