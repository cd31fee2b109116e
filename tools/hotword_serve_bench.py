"""Contextual serving with a hotword list per connection: 16 decoder threads on ONE handle of the full-size contextual + timestamp
model (the C4 configuration bench.py builds), every thread with its own list of 20-50 hotwords, through pfhip_offline_forward —
the call ParaformerHip::Forward makes — with the adapter's defaults (3 execution contexts, 3000 us gather window, 96 utterances).
Two workloads: short utterances of 5-10 s (48 per thread), and VAD-segmented long audio (per thread one 10-minute file cut into
segments of 2-15 s, served in order with the connection's list, as the offline server does).  One JSON line per workload: audio-s/s,
calls per packed forward, bank hit rate.  --merge 0 keeps contextual callers out of the merge queue (what a build without
per-utterance sets does); PFHIP_LIB=<other build> times that build (it has no bank: the hit rate is then reported as null)."""
import argparse
import importlib
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
from conftest import synth_pcm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--merge", type=int, default=1)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--wait-us", type=int, default=3000)
    ap.add_argument("--short-per-thread", type=int, default=48)
    ap.add_argument("--long-seconds", type=int, default=600)
    ap.add_argument("--small", action="store_true", help="a 2-layer model instead of the full-size one (checking the tool itself)")
    args = ap.parse_args()
    pkg = ge.load_package()
    wt = importlib.import_module(pkg.__name__ + ".weights")
    cfg = (wt.small_config(enc_layers=2, dec_layers=2, vocab=400, contextual=1, timestamp=1) if args.small
           else dict(wt.PARAFORMER_LARGE, contextual=1, timestamp=1))
    man, blob = wt.synth_weights(cfg, seed=1234)
    h = pkg.ParaformerHip().InitAsr((man, blob))
    have_bank = hasattr(h._lib, "pfhip_hotword_bank_stats")
    h.set_inflight(args.inflight)
    h.set_batching(args.wait_us, 96)
    if have_bank:
        h.set_hotword_merging(bool(args.merge))
    rng = np.random.default_rng(0)
    T = args.threads
    lists = [h.CompileHotwordEmbedding([list(rng.integers(2, cfg["vocab"], int(rng.integers(2, 8)))) for _ in range(int(rng.integers(20, 51)))])
             for _ in range(T)]
    pool = [synth_pcm(i, 16000 * 15, rng) for i in range(8)]           # cut to length per request
    short = [[int(rng.integers(16000 * 5, 16000 * 10)) for _ in range(args.short_per_thread)] for _ in range(T)]
    longs = []
    for _ in range(T):
        left, segs = 16000 * args.long_seconds, []
        while left > 16000 * 2:
            n = int(min(left, rng.integers(16000 * 2, 16000 * 15)))
            segs.append(n)
            left -= n
        longs.append(segs)
    h.forward_ids([pool[0][:16000 * 8]] * 4, hw_emb=lists[0], want_timestamps=True)          # sizes a workspace, loads code objects

    def run(name, work):
        s0 = h.inflight_stats()
        b0 = h.hotword_bank_stats() if have_bank else None
        err = []

        def serve(t):
            try:
                for k, n in enumerate(work[t]):
                    h.forward_ids([pool[(t + k) % len(pool)][:n]], hw_emb=lists[t], want_timestamps=True)
            except Exception as e:
                err.append(repr(e))
        ths = [threading.Thread(target=serve, args=(t,)) for t in range(T)]
        t0 = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        dt = time.perf_counter() - t0
        s1 = h.inflight_stats()
        fw = sum(a["forwards"] - b["forwards"] for a, b in zip(s1, s0))
        calls = sum(a["calls"] - b["calls"] for a, b in zip(s1, s0))
        audio = sum(sum(w) for w in work) / 16000.0
        res = dict(workload=name, threads=T, merge=args.merge, audio_s=round(audio, 1), wall_s=round(dt, 4), audio_s_per_s=round(audio / dt, 1),
                   calls=calls, forwards=fw, calls_per_forward=round(calls / max(fw, 1), 3), bank_hit_rate=None, errors=err[:3])
        if have_bank:
            b1 = h.hotword_bank_stats()
            hits, miss = b1["hits"] - b0["hits"], b1["misses"] - b0["misses"]
            res.update(bank_hit_rate=round(hits / max(hits + miss, 1), 4), bank_misses=miss, bank_evictions=b1["evictions"] - b0["evictions"],
                       bank_bytes_in_use=b1["bytes_in_use"], sets_per_forward=round((b1["sets_in_forwards"] - b0["sets_in_forwards"]) /
                                                                                    max(b1["forwards"] - b0["forwards"], 1), 3))
        print(json.dumps(res), flush=True)

    run("short_5_10s", short)
    run("long_audio_vad_segments", longs)
    h.close()


if __name__ == "__main__":
    main()
