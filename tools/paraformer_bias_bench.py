#!/usr/bin/env python3
"""Cost of the hotword-biased beam search beside the Paraformer forward ("Hotwords for any Paraformer").

Workload: 32 utterances of 30 s on weights.PARAFORMER_LARGE, synthetic weights and audio (the batch bench.py measures).  Per step,
alternating in one session and each timed on the wall clock (every call ends with its own stream synchronisation, so wall time is
device time plus the call's host work):
  nbest          pfhip_offline_forward_nbest at k = 8 — the forward the search rides on, without it
  bias           pfhip_offline_forward_bias at width 8, beam 16, nbest 1, det->nbest_k = 8, no graph
  bias_hotwords  the same with a graph of --hotwords random hotwords
The baseline of another build (the parent commit's library) is the same `nbest` form run with PFHIP_LIB=<that libpfhip.so> and
--only-nbest in a process of its own (one process holds one libpfhip.so), interleaved with runs of this one in the same session.
The head class of the profile slots (K_HEAD: the top-k head, plus the search in the bias forms) is read in a run of its own after
the timed steps, and the search kernel is timed alone through the operator entry on candidates of the batch's shape (device events
around `reps` launches after warm-up).

Prints one JSON line: medians, minima and maxima in ms.

  python tools/paraformer_bias_bench.py [--batch 32] [--seconds 30] [--steps 6] [--warmup 2] [--reps 20] [--hotwords 1000]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hotwords", type=int, default=1000)
    ap.add_argument("--only-nbest", action="store_true", help="time the nbest form alone (what a parent library can run)")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    from conftest import synth_pcm
    pkg = ge.load_package()
    weights = importlib.import_module("asr_2pass_amd.weights")
    cfg = dict(weights.PARAFORMER_LARGE)
    man, blob = weights.synth_weights(cfg, seed=1234)
    model = pkg.ParaformerHip().InitAsr((man, blob), device=0)
    V = model.vocab_size
    n = int(args.seconds * 16000)
    utts = [synth_pcm(b, n, np.random.default_rng(7000 + b)) for b in range(args.batch)]
    rng = np.random.default_rng(3)
    words = [[int(t) for t in rng.integers(1, V, size=rng.integers(2, 7))] for _ in range(args.hotwords)]
    graph = pkg.ContextGraph(words, [float(rng.integers(1, 9)) / 4 for _ in words], V)
    forms = {"nbest": lambda: model.forward_ids(utts, nbest=8)}
    if not args.only_nbest:
        forms["bias"] = lambda: model.forward_bias(utts, [(8, 16, 1, None)], nbest=8)
        forms["bias_hotwords"] = lambda: model.forward_bias(utts, [(8, 16, 1, graph)], nbest=8)
    t = {k: [] for k in forms}
    got = {}
    for step in range(args.warmup + max(args.steps, 1)):
        for name, fn in forms.items():
            t0 = time.perf_counter()
            got[name] = fn()
            t1 = time.perf_counter()
            if step >= args.warmup:
                t[name].append(1e3 * (t1 - t0))
    rows = [int(min(a, b)) for a, b in zip(got["nbest"]["token_num"], got["nbest"]["n_fires"])]
    res = {"library": os.path.realpath(pkg.LIB_PATH), "batch": args.batch, "seconds": args.seconds, "steps": args.steps, "warmup": args.warmup,
           "token_rows": int(sum(rows)), "longest": int(max(rows)), "hotwords": args.hotwords}
    for name in forms:
        res[name] = stats(t[name])
    if not args.only_nbest:
        res["graph_states"] = int(len(graph.dump()["escape"]))
        for name in ("bias", "bias_hotwords"):
            for b in range(args.batch):
                assert np.array_equal(got[name]["ids"][b], got["nbest"]["ids"][b])
        res["greedy_kept_without_graph"] = bool(all(np.array_equal(got["bias"]["hyps"][b][0][0], got["nbest"]["ids"][b]) for b in range(args.batch)
                                                    if rows[b]))
        res["hotword_ctx_nonzero"] = int(sum(1 for h in got["bias_hotwords"]["hyps"] if h and h[0][3] != 0))
        # the head class of the profile slots, in a run of its own
        model.profile_enable(1)
        for name, fn in forms.items():
            model.profile_read(reset=True)
            for _ in range(3):
                fn()
            res[name]["head_class_ms_per_forward"] = round(model.profile_read(reset=True)["head"]["ms"] / 3, 4)
        model.profile_enable(0)
        # the search kernel alone, on candidates of that batch's shape
        ops = importlib.import_module("asr_2pass_amd.ops")
        B, ML = args.batch, int(sum(rows))
        cand_ids = torch.from_numpy(np.stack([rng.permutation(V)[:8] for _ in range(max(ML, 1))]).astype(np.int32)).cuda()
        cand_lp = torch.from_numpy(-np.cumsum(rng.uniform(0.05, 0.6, size=(max(ML, 1), 8)), axis=1).astype(np.float32)).cuda()
        row_off = torch.tensor(np.concatenate([[0], np.cumsum(rows)])[:-1].tolist(), dtype=torch.int32, device="cuda")
        length = torch.tensor(rows, dtype=torch.int32, device="cuda")

        def timed(fn):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return round(e0.elapsed_time(e1) / args.reps, 4)

        for name, g in (("search_ms", None), ("search_hotwords_ms", graph)):
            res[name] = timed(lambda: ops.nbest_ctx_beam(cand_ids, cand_lp, row_off, length, V, [8] * B, [16] * B, [1] * B,
                                                         graph_of=[-1 if g is None else 0] * B, graphs=[] if g is None else [g],
                                                         max_tokens=max(rows), rows=ML))
    print(json.dumps(res), flush=True)
    model.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
