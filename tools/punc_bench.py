#!/usr/bin/env python3
"""Wall time of the punctuation calls on the two CT-Transformer shapes ("The large CT-Transformer").

Synthetic weights, vocabulary 5000: `small` = 256 / 8 / 1024 x 4 (d_k = 32, attention.hip's kernel), `large` = 516 / 12 / 2048 x 12
(d_k = 43, its exact-width form).  Three loads per model: Infer of 20 ids, Infer of 200 ids, pfhip_punc_infer_batch of 32 x 40 ids.
Per load, warm-up calls and then timed calls with the models alternating call by call, so that clock and thermal drift hit both
alike.  Wall time per call includes the upload of the ids and the download of the punctuation ids.

Prints one JSON line: per model and load the median, minimum and maximum in ms, and the kernel launches of one call
(1 gather + 8 per block + LayerNorm, head GEMM and arg-max).  A library that cannot create a model (a build from before the
large model was served, chosen with PFHIP_LIB) reports the refusal for it and times the rest.

  python tools/punc_bench.py [--models small,large] [--steps 50] [--warmup 5]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOCAB = 5000
SHAPES = {"small": dict(d_model=256, n_head=8, ffn=1024, layers=4), "large": dict(d_model=516, n_head=12, ffn=2048, layers=12)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="small,large")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    weights = importlib.import_module("asr_2pass_amd.weights")
    res = {"library": os.path.realpath(pkg.LIB_PATH), "vocab": VOCAB, "steps": max(args.steps, 1), "warmup": max(args.warmup, 1), "models": {}}
    handles = {}
    for name in args.models.split(","):
        cfg = dict(weights.CT_TRANSFORMER, vocab=VOCAB, **SHAPES[name])
        man, blob = weights.synth_punc_weights(cfg, seed=1234)
        res["models"][name] = {"shape": SHAPES[name], "kernel_launches_per_call": 1 + 8 * cfg["layers"] + 3}
        try:
            handles[name] = pkg.CTTransformerHip().InitPunc((man, blob))
        except pkg.PfhipError as e:
            if getattr(e, "status", None) != 4:          # PFHIP_ERR_UNSUPPORTED: the shape; anything else (no device) is a failure
                raise
            res["models"][name]["refused"] = str(e)
    rng = np.random.default_rng(20251114)
    one = lambda n: rng.integers(0, VOCAB, n).astype(np.int32)
    ids20, ids200, batch = one(20), one(200), [one(40) for _ in range(32)]
    loads = {"infer_20": lambda h: h.Infer(ids20), "infer_200": lambda h: h.Infer(ids200), "infer_batch_32x40": lambda h: h.InferBatch(batch)}
    for load, call in loads.items():
        for _ in range(res["warmup"]):
            for h in handles.values():
                call(h)
        ms = {name: [] for name in handles}
        for _ in range(res["steps"]):
            for name, h in handles.items():          # interleaved
                t0 = time.perf_counter()
                call(h)
                ms[name].append(1e3 * (time.perf_counter() - t0))
        for name, v in ms.items():
            res["models"][name][load] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    print(json.dumps(res), flush=True)
    for h in handles.values():
        h.close()
    return 0 if handles or all("refused" in m for m in res["models"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
