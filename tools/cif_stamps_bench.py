#!/usr/bin/env python3
"""What time stamps from the CIF scan cost, and what they save where the timestamp head exists ("Offline: time
stamps from the CIF scan").

One process, the C4 batch (32 x 30 s, tools/c4_bench.py's synthetic audio, synthetic Paraformer-large) from HOST buffers, two
comparisons, each with its two forms alternating step by step as tools/pcm16_bench.py does, so that clock and thermal drift hit both
alike.  Wall time per call: H2D of the audio + the forward + D2H of the results + the host rule that makes the spans.

  plain model       off: pfhip_offline_forward                          fires: pfhip_offline_forward_detail with fire_frame
                                                                               + pfhip_cif_timestamps per utterance
                                                                        fires_only: the same call without the host rule (what
                                                                               the device and the C ABI add; the rule's calls are
                                                                               made from Python here)
  timestamp model   head (mode 0): pfhip_offline_forward with us_alphas / us_peaks + pfhip_timestamp_onnx per utterance
                    cif  (mode 2): pfhip_offline_forward_detail with fire_frame, the three us_* NULL (the head is skipped)
                                   + pfhip_cif_timestamps per utterance

Prints one JSON line: ms per batch (median, min, max) of every series, the run-to-run spread of each comparison's first series
(max - min and the standard deviation), the differences of the medians to that first series, and whether ids / token_num / n_fires
of the forms of a comparison are identical (they must be).

  python tools/cif_stamps_bench.py [--steps 20] [--warmup 2] [--batch 32] [--seconds 30]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

SR = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=int, default=30)
    args = ap.parse_args()
    import __graft_entry__ as ge
    from conftest import synth_pcm
    pkg = ge.load_package()
    wt = importlib.import_module("asr_2pass_amd.weights")
    lib = pkg.load_lib()
    B, n = args.batch, args.seconds * SR
    rng = np.random.default_rng(0)
    waves = [np.ascontiguousarray(synth_pcm(i, n, rng)) for i in range(B)]
    lens = (ctypes.c_int * B)(*([n] * B))
    ptrs = (ctypes.c_void_p * B)(*[w.ctypes.data for w in waves])
    sof = (ctypes.c_int * B)(*([0] * B))
    max_tokens = n // 960 + 2
    max_us = 3 * max_tokens
    i32p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)

    def prepared(with_us, with_fire):
        p = dict(ids=np.zeros((B, max_tokens), np.int32), tn=np.zeros(B, np.int32), nf=np.zeros(B, np.int32), fr=np.zeros(B, np.int32),
                 spans=np.zeros((2 * max_tokens + 4, 3), np.float32))
        out = pkg._Out()
        out.token_ids, out.token_num = p["ids"].ctypes.data_as(i32p), p["tn"].ctypes.data_as(i32p)
        out.n_fires, out.n_frames = p["nf"].ctypes.data_as(i32p), p["fr"].ctypes.data_as(i32p)
        out.logp = None
        out.max_tokens = max_tokens
        if with_us:
            p["usa"], p["usp"], p["usl"] = np.zeros((B, max_us), np.float32), np.zeros((B, max_us), np.float32), np.zeros(B, np.int32)
            out.us_alphas, out.us_peaks, out.us_len = p["usa"].ctypes.data_as(f32p), p["usp"].ctypes.data_as(f32p), p["usl"].ctypes.data_as(i32p)
            out.max_us = max_us
        if with_fire:
            p["fire"] = np.full((B, max_tokens), -1, np.int32)
            p["det"] = pkg._Detail(0, None, None, p["fire"].ctypes.data_as(i32p))
        p["out"] = out
        return p

    def check(st, what):
        if st != 0:
            raise SystemExit(f"{what}: pfhip status {st}: {lib.pfhip_last_error().decode()}")

    def run_plain(h, p, hw):
        check(lib.pfhip_offline_forward(h, ptrs, lens, B, hw[0], hw[1], ctypes.byref(p["out"])), "forward")
        return 0

    def run_head(h, p, hw):
        check(lib.pfhip_offline_forward(h, ptrs, lens, B, hw[0], hw[1], ctypes.byref(p["out"])), "forward + head")
        k, n_spans = 0, ctypes.c_int(0)
        for b in range(B):
            nt = int(min(p["tn"][b], p["nf"][b]))
            if nt > 1:
                check(lib.pfhip_timestamp_onnx(p["usa"][b].ctypes.data, p["usp"][b].ctypes.data, int(p["usl"][b]), nt - 1, 0.0, -1.5,
                                               p["spans"].ctypes.data, p["spans"].shape[0], ctypes.byref(n_spans)), "timestamp_onnx")
                k += n_spans.value
        return k

    def run_cif(h, p, hw, rule=True):
        sets = (ctypes.c_void_p * 1)(hw[0])
        rows = (ctypes.c_int * 1)(hw[1])
        check(lib.pfhip_offline_forward_detail(h, ptrs, lens, B, 0, sets, rows, 1 if hw[1] else 0, sof, ctypes.byref(p["out"]),
                                               ctypes.byref(p["det"])), "forward_detail")
        k, n_spans = 0, ctypes.c_int(0)
        for b in range(B if rule else 0):
            nt = int(min(p["tn"][b], p["nf"][b]))
            if nt > 1:
                check(lib.pfhip_cif_timestamps(p["fire"][b].ctypes.data, nt, nt - 1, int(p["fr"][b]), 60.0, 0.0, p["spans"].ctypes.data,
                                               p["spans"].shape[0], ctypes.byref(n_spans)), "cif_timestamps")
                k += n_spans.value
        return k

    res = {"workload": f"{B} x {args.seconds} s synthetic 16 kHz, Paraformer-large, host buffers in, ids and spans out",
           "steps": max(args.steps, 1), "warmup": max(args.warmup, 1)}
    plans = (("plain", {}, (("off", run_plain, (False, False)), ("fires", run_cif, (False, True)),
                            ("fires_only", lambda h, p, hw: run_cif(h, p, hw, rule=False), (False, True)))),
             ("timestamp", dict(timestamp=1), (("head", run_head, (True, False)), ("cif", run_cif, (False, True)))))
    ok = True
    for model_name, over, forms in plans:
        man, blob = wt.synth_weights(dict(wt.PARAFORMER_LARGE, **over), seed=1234)
        model = pkg.ParaformerHip().InitAsr((man, blob), device=0)
        h, hw = model.handle, (None, 0)
        prep = {name: prepared(*flags) for name, _, flags in forms}
        ms = {name: [] for name, _, _ in forms}
        spans = {}

        def step(name, fn):
            t0 = time.perf_counter()
            spans[name] = fn(h, prep[name], hw)
            return 1e3 * (time.perf_counter() - t0)
        for _ in range(max(args.warmup, 1)):
            for name, fn, _ in forms:
                step(name, fn)
        for _ in range(max(args.steps, 1)):
            for name, fn, _ in forms:           # interleaved
                ms[name].append(step(name, fn))
        a_name = forms[0][0]
        a = prep[a_name]
        same = all(bool(np.array_equal(a["tn"], prep[n]["tn"]) and np.array_equal(a["nf"], prep[n]["nf"]) and
                        np.array_equal(a["ids"], prep[n]["ids"])) for n, _, _ in forms[1:])
        ok = ok and same
        r = {"ids_identical": same, "tokens": int(a["nf"].sum())}
        for name, _, _ in forms:
            v = ms[name]
            r[name] = {"ms_per_batch_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3),
                       "spans": spans[name]}
        v = ms[a_name]
        r[a_name + "_spread_ms"] = {"max_minus_min": round(max(v) - min(v), 3), "stdev": round(statistics.pstdev(v), 3)}
        for b_name, _, _ in forms[1:]:
            r[f"{b_name}_minus_{a_name}_median_ms"] = round(r[b_name]["ms_per_batch_median"] - r[a_name]["ms_per_batch_median"], 3)
        res[model_name] = r
        model.close()
    print(json.dumps(res), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
