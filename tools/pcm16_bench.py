#!/usr/bin/env python3
"""What 16-bit PCM in buys at the host boundary ("16-bit PCM in").

One process, one handle: the headline batch (32 x 30 s, bench.py's synthetic audio and synthetic Paraformer-large) from HOST
buffers through pfhip_offline_forward (float32 samples, 4 bytes each across the bus) and through pfhip_offline_forward_s16 (the
int16 samples the floats were made from, 2 bytes each), the two alternating step by step so that clock and thermal drift hit both
alike.  Wall time per call: H2D of the audio + the forward + D2H of the ids, as the reference times its own batch
(paraformer-torch.cpp:355-358 has the copy inside).  Output buffers are allocated once outside the timed calls.

Prints one JSON line: ms per batch (median, min, max) of both series, the H2D bytes of each, the run-to-run spread of the f32
series (max - min and the standard deviation), and whether the ids of the two forms are identical (they must be).

  python tools/pcm16_bench.py [--steps 20] [--warmup 1] [--batch 32] [--seconds 30]
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

SR = 16000
SEED_PCM = 20251114          # bench.py's


def synth_s16(index, n, rng):
    """bench.py's utterance before its division by 32768: s16 = round(8000 (0.6 sin(2 pi f_i t) + 0.4 N(0,1)))."""
    t = np.arange(n, dtype=np.float64) / SR
    f = 110.0 * 2.0 ** ((index % 24) / 12.0)
    x = 8000.0 * (0.6 * np.sin(2 * np.pi * f * t) + 0.4 * rng.standard_normal(n))
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=int, default=30)
    args = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    weights = importlib.import_module("asr_2pass_amd.weights")
    man, blob = weights.synth_weights(dict(weights.PARAFORMER_LARGE), seed=1234)
    model = pkg.ParaformerHip().InitAsr((man, blob), device=0)
    lib, h = pkg.load_lib(), model.handle

    B, n = args.batch, args.seconds * SR
    rng = np.random.default_rng(SEED_PCM)
    s16 = [synth_s16(i, n, rng) for i in range(B)]
    f32 = [(u / 32768.0).astype(np.float32) for u in s16]           # bench.py's floats, bit for bit
    lens = (ctypes.c_int * B)(*([n] * B))
    max_tokens = n // 960 + 2

    def prepared(bufs):
        ids = np.zeros((B, max_tokens), np.int32)
        tn, nf, fr = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
        out = pkg._Out()
        out.token_ids = ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out.token_num = tn.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out.n_fires = nf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out.n_frames = fr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out.logp = None
        out.max_tokens = max_tokens
        ptrs = (ctypes.c_void_p * B)(*[b.ctypes.data for b in bufs])
        return dict(ptrs=ptrs, out=out, ids=ids, tn=tn, nf=nf, keep=(bufs, fr))

    forms = {"f32": (lib.pfhip_offline_forward, prepared(f32)), "s16": (lib.pfhip_offline_forward_s16, prepared(s16))}

    def step(name):
        fn, p = forms[name]
        t0 = time.perf_counter()
        st = fn(h, p["ptrs"], lens, B, None, 0, ctypes.byref(p["out"]))
        dt = time.perf_counter() - t0
        if st != 0:
            raise SystemExit(f"{name}: pfhip status {st}: {lib.pfhip_last_error().decode()}")
        return 1e3 * dt

    for _ in range(max(args.warmup, 1)):
        for name in forms:
            step(name)
    ms = {name: [] for name in forms}
    for _ in range(max(args.steps, 1)):
        for name in forms:                   # interleaved
            ms[name].append(step(name))
    a, b = forms["f32"][1], forms["s16"][1]
    same = bool(np.array_equal(a["tn"], b["tn"]) and np.array_equal(a["nf"], b["nf"]) and np.array_equal(a["ids"], b["ids"]))
    res = {"workload": f"{B} x {args.seconds} s synthetic 16 kHz, Paraformer-large, host buffers in, ids out",
           "steps": len(ms["f32"]), "warmup": max(args.warmup, 1), "ids_identical": same, "tokens": int(a["tn"].sum())}
    for name, es in (("f32", 4), ("s16", 2)):
        v = ms[name]
        med = statistics.median(v)
        res[name] = {"ms_per_batch_median": round(med, 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3),
                     "h2d_bytes": B * n * es, "audio_s_per_s": round(B * args.seconds / (med / 1e3), 1)}
    res["f32_spread_ms"] = {"max_minus_min": round(max(ms["f32"]) - min(ms["f32"]), 3),
                            "stdev": round(statistics.pstdev(ms["f32"]), 3)}
    res["s16_minus_f32_median_ms"] = round(res["s16"]["ms_per_batch_median"] - res["f32"]["ms_per_batch_median"], 3)
    print(json.dumps(res), flush=True)
    model.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
