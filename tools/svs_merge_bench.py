#!/usr/bin/env python3
"""Merged against unmerged SenseVoiceSmall callers ("SenseVoiceSmall: merged callers, spans in one call").

Workload: `--threads` caller threads on ONE handle (weights.SENSEVOICE_SMALL, synthetic weights and audio, PFHIP_INFLIGHT-style
`--inflight` execution contexts), each a stream of `--segments` segments of 2-8 s, one pfhip_svs_forward_spans of batch 1 per segment:
the second pass of the 2-pass flow.  Two settings of the same build are run interleaved, `--rounds` times each: merging on
(pfhip_svs_set_batching(wait_us, max)) and wait_us = 0, which is what a direct caller gets.  Wall clock per call and per round.

Prints one JSON line: per setting the medians over the rounds (with minimum and maximum) of segments per second and of the p50 / p99
call latency in ms, and the forwards / calls of the last round.

  python tools/svs_merge_bench.py [--threads 16] [--segments 6] [--rounds 5] [--wait-us 3000] [--max 96] [--inflight 3]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--segments", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--wait-us", type=int, default=3000)
    ap.add_argument("--max", type=int, default=96)
    ap.add_argument("--inflight", type=int, default=3)
    args = ap.parse_args()
    import __graft_entry__ as ge
    from conftest import synth_pcm
    pkg = ge.load_package()
    weights = importlib.import_module("asr_2pass_amd.weights")
    man, blob = weights.synth_svs_weights(dict(weights.SENSEVOICE_SMALL))
    model = pkg.SenseVoiceHip().InitAsr((man, blob), device=0)
    model.set_inflight(args.inflight)
    rng = np.random.default_rng(99)
    segs = [[np.clip(np.round(synth_pcm(100 * t + i, int(rng.uniform(2.0, 8.0) * 16000), np.random.default_rng(100 * t + i)) * 32768.0),
                     -32768, 32767).astype(np.int16) for i in range(args.segments)] for t in range(args.threads)]
    langs = ["auto", "zh", "en", "yue", "ja", "ko"]
    model.warm_up(8, 8 * 16000)

    def one_round(wait_us):
        model.set_batching(wait_us, args.max)
        gate, lat = threading.Barrier(args.threads + 1), [[] for _ in range(args.threads)]

        def body(t):
            gate.wait()
            for x in segs[t]:
                t0 = time.perf_counter()
                model.forward([x], lang=langs[t % len(langs)], itn=bool(t & 1), want_spans=True)
                lat[t].append(1e3 * (time.perf_counter() - t0))

        ts = [threading.Thread(target=body, args=(t,)) for t in range(args.threads)]
        st0 = model.inflight_stats()
        for th in ts:
            th.start()
        gate.wait()
        t0 = time.perf_counter()
        for th in ts:
            th.join()
        wall = time.perf_counter() - t0
        st1 = model.inflight_stats()
        allv = sorted(v for l in lat for v in l)
        delta = lambda key: sum(s[key] for s in st1) - sum(s[key] for s in st0)
        return dict(seg_per_s=len(allv) / wall, p50=allv[len(allv) // 2], p99=allv[min(len(allv) - 1, int(0.99 * len(allv)))],
                    forwards=delta("forwards"), calls=delta("calls"))

    one_round(args.wait_us)
    one_round(0)                                        # warm both settings
    runs = {"merged": [], "unmerged": []}
    for _ in range(args.rounds):                        # interleaved A/B
        runs["merged"].append(one_round(args.wait_us))
        runs["unmerged"].append(one_round(0))
    res = {"library": os.path.realpath(pkg.LIB_PATH), "threads": args.threads, "segments_per_thread": args.segments, "rounds": args.rounds,
           "wait_us": args.wait_us, "max_utterances": args.max, "inflight": args.inflight}
    for name, rr in runs.items():
        res[name] = {"segments_per_s": spread([r["seg_per_s"] for r in rr]), "p50_ms": spread([r["p50"] for r in rr]),
                     "p99_ms": spread([r["p99"] for r in rr]), "forwards": rr[-1]["forwards"], "calls": rr[-1]["calls"]}
    print(json.dumps(res), flush=True)
    model.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
