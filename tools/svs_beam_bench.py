#!/usr/bin/env python3
"""Cost of the CTC prefix beam search on the device beside the SenseVoiceSmall forward ("SenseVoiceSmall: prefix
beam search and hotwords").

Workload: 32 utterances of 30 s on weights.SENSEVOICE_SMALL (512 / 4 / 2048, 50 + 20 layers, vocabulary 25 055), synthetic weights
and audio.  Per step, alternating in one session and each timed on the wall clock (every call ends with its own stream
synchronisation, so wall time is device time plus the call's host work):
  plain      pfhip_svs_forward
  logp       pfhip_svs_forward with full log-prob rows — what a caller with a decoder handle costs without the device search
             (the unfused head and rows x vocabulary floats to the host; the host's own search over them is not included)
  beam_3     pfhip_svs_forward_beam at 3/3, beam_10 at 10/10, and both again with a graph of --hotwords random hotwords
The two kernels are then timed on their own through the operator entries (device events around `reps` launches after warm-up): the
top-k head on operands of the batch's shape against the greedy head, the search on the k best columns that head left.

Prints one JSON line: medians, minima and maxima in ms, and the bytes each form copies to the host.

  python tools/svs_beam_bench.py [--batch 32] [--seconds 30] [--steps 6] [--warmup 2] [--reps 10] [--hotwords 1000] [--no-logp]
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--hotwords", type=int, default=1000)
    ap.add_argument("--no-logp", action="store_true", help="leave the full-rows form out (it needs rows x vocabulary floats of host memory)")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    from conftest import synth_pcm
    pkg = ge.load_package()
    weights = importlib.import_module("asr_2pass_amd.weights")
    ops = importlib.import_module("asr_2pass_amd.ops")
    cfg = dict(weights.SENSEVOICE_SMALL)
    man, blob = weights.synth_svs_weights(cfg)
    model = pkg.SenseVoiceHip().InitAsr((man, blob), device=0)
    V, d = int(cfg["vocab"]), int(cfg["d_model"])
    n = int(args.seconds * 16000)
    utts = [synth_pcm(b, n, np.random.default_rng(7000 + b)) for b in range(args.batch)]
    rng = np.random.default_rng(3)
    words = [[int(t) for t in rng.integers(1, V, size=rng.integers(2, 7))] for _ in range(args.hotwords)]
    graph = pkg.ContextGraph(words, [float(rng.integers(1, 9)) / 4 for _ in words], V)
    forms = {"plain": {}, "beam_3": dict(beam=(3, 3)), "beam_10": dict(beam=(10, 10)), "beam_3_hotwords": dict(beam=(3, 3), graph=graph),
             "beam_10_hotwords": dict(beam=(10, 10), graph=graph)}
    if not args.no_logp:
        forms["logp"] = dict(want_logp=True)
    t = {k: [] for k in forms}
    got = {}
    for step in range(args.warmup + max(args.steps, 1)):
        for name, kw in forms.items():
            t0 = time.perf_counter()
            got[name] = model.forward(utts, lang="auto", itn=False, **kw)
            t1 = time.perf_counter()
            if step >= args.warmup:
                t[name].append(1e3 * (t1 - t0))
    rows = [int(r) for r in got["plain"]["frame_len"]]
    M, B, maxT = sum(rows), args.batch, max(rows)
    base_bytes = 4 * (B + 3 * B * maxT + 2 * M)
    res = {"library": os.path.realpath(pkg.LIB_PATH), "batch": B, "seconds": args.seconds, "steps": args.steps, "warmup": args.warmup,
           "rows": M, "hotwords": args.hotwords, "graph_states": int(len(graph.dump()["escape"]))}
    for name in forms:
        res[name] = stats(t[name])
    res["bytes_to_host"] = {"plain": base_bytes, "logp": base_bytes + 4 * M * V,
                            "beam_3": base_bytes + 4 * (B + B * 3 * (4 + maxT - 4)), "beam_10": base_bytes + 4 * (B + B * 10 * (4 + maxT - 4))}
    res["beam_tokens_best"] = int(sum(len(h[0]) for h in got["beam_10"]["beam_ids"] if len(h)))
    res["hotword_ctx_nonzero"] = int(sum(1 for s in got["beam_10_hotwords"]["beam_ctx_score"] if len(s) and s[0] != 0))

    # the kernels alone, on the shapes of that batch
    g = np.random.default_rng(1)
    X = torch.from_numpy(g.standard_normal((M, d)).astype(np.float32)).cuda()
    W = torch.from_numpy((g.standard_normal((V, d)) / np.sqrt(d)).astype(np.float32)).cuda()
    bias = torch.zeros(V, dtype=torch.float32, device="cuda")
    ws = ops.best_w_scale(float(W.abs().max()))
    row_off = torch.tensor((np.concatenate([[0], np.cumsum(rows)])[:-1] + 4).tolist(), dtype=torch.int32, device="cuda")
    length = torch.tensor([r - 4 for r in rows], dtype=torch.int32, device="cuda")

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

    res["head_greedy_ms"] = timed(lambda: ops.ctc_head(X, W, bias, w_scale=ws))
    for k in (3, 10):
        res[f"head_topk_{k}_ms"] = timed(lambda: ops.ctc_head_topk(X, W, bias, k, w_scale=ws))
        _, _, _, tk_ids, tk_lp = ops.ctc_head_topk(X, W, bias, k, w_scale=ws)
        res[f"search_{k}_ms"] = timed(lambda: ops.ctc_prefix_beam(tk_ids, tk_lp, row_off, length, V, k, k, nbest=k, max_tokens=maxT))
        res[f"search_{k}_hotwords_ms"] = timed(lambda: ops.ctc_prefix_beam(tk_ids, tk_lp, row_off, length, V, k, k, nbest=k, max_tokens=maxT,
                                                                        graph=graph))
    print(json.dumps(res), flush=True)
    model.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
