#!/usr/bin/env python3
"""Cost of the CTC forced alignment beside the SenseVoiceSmall forward it follows ("SenseVoiceSmall: forced
alignment").

Workload: 32 utterances of 30 s on weights.SENSEVOICE_SMALL (512 / 4 / 2048, 50 + 20 layers, vocabulary 25 055), synthetic weights
and audio.  Each step runs one forward and then pfhip_svs_align on that forward's greedy tokens (the collapse of its speech rows), the
two timed separately on the wall clock: both calls end with their own stream synchronisation, so wall time is device time plus the
call's host work.  The two kernels are then timed on their own through the operator entries on buffers of the same shapes and labels
(device events around `reps` launches in a row, after warm-up launches), which gives their shares of the call.

Prints one JSON line: medians, minima and maxima in ms, the rows / tokens / states of the batch and align_over_forward.

--in-forward adds the A/B of the one-call form: per step, interleaved, (A) forward + pfhip_svs_align on ids[b][4:] against (B)
pfhip_svs_forward_spans, which forms the same spans inside the forward; "two_calls" / "one_call" in the JSON, wall clock.

  python tools/svs_align_bench.py [--batch 32] [--seconds 30] [--steps 10] [--warmup 3] [--reps 20] [--in-forward]
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


def collapse(frame_ids, blank):
    out, prev = [], -1
    for x in frame_ids:
        x = int(x)
        if x != blank and x != prev:
            out.append(x)
        prev = x
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--in-forward", action="store_true")
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
    blank = int(cfg["blank_id"])
    n = int(args.seconds * 16000)
    utts = [synth_pcm(b, n, np.random.default_rng(7000 + b)) for b in range(args.batch)]
    t_fwd, t_al = [], []
    for step in range(args.warmup + max(args.steps, 1)):
        t0 = time.perf_counter()
        got = model.forward(utts, lang="auto", itn=False)
        t1 = time.perf_counter()
        tokens = [collapse(f[4:], blank) for f in got["frame_ids"]]
        t2 = time.perf_counter()
        al = model.align(tokens)
        t3 = time.perf_counter()
        if step >= args.warmup:
            t_fwd.append(1e3 * (t1 - t0))
            t_al.append(1e3 * (t3 - t2))
    rows = [int(r) for r in got["frame_len"]]
    res = {"library": os.path.realpath(pkg.LIB_PATH), "batch": args.batch, "seconds": args.seconds, "steps": len(t_fwd), "warmup": args.warmup,
           "rows": sum(rows), "speech_rows_max": max(rows) - 4, "tokens": sum(len(y) for y in tokens), "tokens_max": max(len(y) for y in tokens),
           "feasible": int(np.isfinite(al["score"]).sum()), "forward": stats(t_fwd), "align": stats(t_al)}
    res["align_over_forward"] = round(res["align"]["ms_median"] / res["forward"]["ms_median"], 4)

    if args.in_forward:
        t_two, t_one = [], []
        for step in range(args.warmup + max(args.steps, 1)):
            t0 = time.perf_counter()
            got = model.forward(utts, lang="auto", itn=False)
            al = model.align([ids[4:] for ids in got["ids"]])
            t1 = time.perf_counter()
            one = model.forward(utts, lang="auto", itn=False, want_spans=True)
            t2 = time.perf_counter()
            if step >= args.warmup:
                t_two.append(1e3 * (t1 - t0))
                t_one.append(1e3 * (t2 - t1))
        res["two_calls"], res["one_call"] = stats(t_two), stats(t_one)
        res["spans_equal"] = bool(all(np.array_equal(a, b) for a, b in zip(al["begin"], one["span_begin"])) and
                                  all(np.array_equal(a, b) for a, b in zip(al["end"], one["span_end"])))
        res["span_tokens"] = int(sum(len(x) for x in one["span_begin"]))

    # the two kernels alone, on the shapes and labels of that batch
    d, V = int(cfg["d_model"]), int(cfg["vocab"])
    M = sum(rows)
    rng = np.random.default_rng(1)
    X = torch.from_numpy(rng.standard_normal((M, d)).astype(np.float32)).cuda()
    W = torch.from_numpy((rng.standard_normal((V, d)) / np.sqrt(d)).astype(np.float32)).cuda()
    bias = torch.zeros(V, dtype=torch.float32, device="cuda")
    lse = torch.full((M,), 10.0, dtype=torch.float32, device="cuda")
    row_off = torch.tensor((np.concatenate([[0], np.cumsum(rows)])[:-1] + 4).tolist(), dtype=torch.int32, device="cuda")
    lab = ops.CtcLabels(tokens, [r - 4 for r in rows])
    E = ops.ctc_emissions(X, W, bias, lse, row_off, lab, blank=blank)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / args.reps, 4)

    res["emissions_kernel_ms"] = timed(lambda: ops.ctc_emissions(X, W, bias, lse, row_off, lab, blank=blank, E=E))
    res["viterbi_kernel_ms"] = timed(lambda: ops.ctc_align(E, lab))
    res["e_floats"] = lab.e_floats
    print(json.dumps(res), flush=True)
    model.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
