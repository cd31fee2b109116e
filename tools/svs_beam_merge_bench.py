#!/usr/bin/env python3
"""Merged against unmerged SenseVoiceSmall BEAM callers ("SenseVoiceSmall: merged beam callers, one graph each").

Workload: `--threads` caller threads on ONE handle (weights.SENSEVOICE_SMALL, synthetic weights and audio, `--inflight` execution
contexts), each a connection with its OWN hotword graph of `--hotwords` random words, each a stream of `--segments` segments of
2-8 s, one pfhip_svs_forward_beam of batch 1 per segment with beams `--beam` / `--beam`: what a server's decoder thread calls.  Two
settings of the same build are run interleaved, `--rounds` times each: beam merging on (pfhip_svs_set_beam_merging with
pfhip_svs_set_batching(wait_us, max)) and off, where every beam call is a forward of its own with its graph uploaded by the call —
the library's behaviour before the switch existed.  Wall clock per call and per round.

Prints one JSON line: per setting the medians over the rounds (with minimum and maximum) of segments per second and of the p50 / p99
call latency in ms, the forwards / calls of the last round (calls per forward), and the graph bank's hits / misses over the run.

  python tools/svs_beam_merge_bench.py [--threads 16] [--segments 6] [--rounds 5] [--hotwords 20] [--beam 3] [--wait-us 3000]
                                       [--max 96] [--inflight 3]
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
    ap.add_argument("--hotwords", type=int, default=20)
    ap.add_argument("--beam", type=int, default=3)
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
    V = int(model.cfg["vocab"])
    rng = np.random.default_rng(99)
    segs = [[np.clip(np.round(synth_pcm(100 * t + i, int(rng.uniform(2.0, 8.0) * 16000), np.random.default_rng(100 * t + i)) * 32768.0),
                     -32768, 32767).astype(np.int16) for i in range(args.segments)] for t in range(args.threads)]
    graphs = []
    for t in range(args.threads):                       # every connection its own list: 2-6 tokens a word, a weight per word
        g = np.random.default_rng(5000 + t)
        words = [[int(x) for x in g.integers(1, V, size=g.integers(2, 7))] for _ in range(args.hotwords)]
        graphs.append(pkg.ContextGraph(words, [float(g.integers(1, 9)) / 4 for _ in words], V))
    langs = ["auto", "zh", "en", "yue", "ja", "ko"]
    model.warm_up(8, 8 * 16000)

    def one_round(merge):
        model.set_batching(args.wait_us, args.max)
        model.set_beam_merging(merge)
        gate, lat = threading.Barrier(args.threads + 1), [[] for _ in range(args.threads)]

        def body(t):
            gate.wait()
            for x in segs[t]:
                t0 = time.perf_counter()
                model.forward([x], lang=langs[t % len(langs)], itn=bool(t & 1), beam=(args.beam, args.beam), nbest=1, graph=graphs[t])
                lat[t].append(1e3 * (time.perf_counter() - t0))

        ts = [threading.Thread(target=body, args=(t,)) for t in range(args.threads)]
        st0, b0 = model.inflight_stats(), model.graph_bank_stats()
        for th in ts:
            th.start()
        gate.wait()
        t0 = time.perf_counter()
        for th in ts:
            th.join()
        wall = time.perf_counter() - t0
        st1, b1 = model.inflight_stats(), model.graph_bank_stats()
        allv = sorted(v for l in lat for v in l)
        delta = lambda key: sum(s[key] for s in st1) - sum(s[key] for s in st0)
        return dict(seg_per_s=len(allv) / wall, p50=allv[len(allv) // 2], p99=allv[min(len(allv) - 1, int(0.99 * len(allv)))],
                    forwards=delta("forwards"), calls=delta("calls"), bank_hits=b1["hits"] - b0["hits"], bank_misses=b1["misses"] - b0["misses"])

    one_round(True)
    one_round(False)                                    # warm both settings
    runs = {"merged": [], "unmerged": []}
    for _ in range(args.rounds):                        # interleaved A/B
        runs["merged"].append(one_round(True))
        runs["unmerged"].append(one_round(False))
    res = {"library": os.path.realpath(pkg.LIB_PATH), "threads": args.threads, "segments_per_thread": args.segments, "rounds": args.rounds,
           "hotwords": args.hotwords, "beam": args.beam, "wait_us": args.wait_us, "max_utterances": args.max, "inflight": args.inflight,
           "graph_bank": model.graph_bank_stats()}
    for name, rr in runs.items():
        res[name] = {"segments_per_s": spread([r["seg_per_s"] for r in rr]), "p50_ms": spread([r["p50"] for r in rr]),
                     "p99_ms": spread([r["p99"] for r in rr]), "forwards": rr[-1]["forwards"], "calls": rr[-1]["calls"],
                     "calls_per_forward": round(rr[-1]["calls"] / max(rr[-1]["forwards"], 1), 2),
                     "bank_hits": sum(r["bank_hits"] for r in rr), "bank_misses": sum(r["bank_misses"] for r in rr)}
    print(json.dumps(res), flush=True)
    model.set_beam_merging(False)
    model.set_batching(0, args.max)
    for g in graphs:
        g.close()
    model.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
