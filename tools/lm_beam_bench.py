#!/usr/bin/env python3
"""What a token n-gram language model costs inside the two device searches ("Token n-gram LM in the device
searches").

One process: the two search launches on candidate rows shaped like the headline batch (32 utterances x 30 s: 500 rows each) —
pfhip_op_ctc_prefix_beam_multi[_lm] over the k best columns of a CTC head (vocabulary 25055, beams 10 / 10) and
pfhip_op_nbest_ctx_beam[_lm] over the candidates of a Paraformer head (vocabulary 8404, width 8, beam 16) — each without a model
and with a synthetic 4-gram of about 10^6 n-grams built through pfhip_lm_graph_create, the two alternating step by step so that
clock and thermal drift hit both alike.  Rows are random with a peaked first column; the model's n-grams are random too, so most
steps miss their state's arcs and walk the back-off chain to the unigrams: the expensive case.  Time per launch from device events
around the entry (its one host-to-device copy of descriptors and images included, as a forward pays it).

Then the forwards that contain those launches, on the synthetic full-size models and bench.py's synthetic audio (32 x 30 s, host
buffers in, results out, wall time per call): SenseVoiceSmall's forward with the 10 / 10 search and Paraformer-large's forward with
the width-8 / beam-16 search, each without a model and after pfhip_set_token_lm of the same 4-gram, alternating the same way
(--no-forward skips them).

Prints one JSON line: ms per launch / per batch (median, min, max, standard deviation) of every series and the model's size.
A library without the model entries (PFHIP_LIB pointing at an older build) runs the no-model series alone, and so does --no-model
with this one: the A/B of the two builds compares those, since a model series in between (a 20 MB image through the caches every
other step) is company the older build's series does not have.

  python tools/lm_beam_bench.py [--steps 20] [--warmup 3] [--batch 32] [--rows 500] [--seconds 30] [--forward-steps 6] [--no-forward] [--no-model]
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_4gram(lib, V, seed, sizes=(400000, 350000, 250000)):
    """A prefix-closed random 4-gram over V tokens, </s> (V) and <s> (V + 1): every unigram, then sizes[n - 2] distinct n-grams whose
    history is a listed (n - 1)-gram.  Returns (handle, n-gram count)."""
    rng = np.random.default_rng(seed)
    level = np.concatenate([np.arange(V, dtype=np.int32), [V, V + 1]]).astype(np.int32).reshape(-1, 1)
    counts, labels, n_all = [], [], 0
    for n in range(1, 5):
        if n > 1:
            hist = level[level[:, -1] != V]                          # nothing follows </s>
            pick = hist[rng.integers(0, len(hist), size=sizes[n - 2])]
            nxt = rng.integers(0, V + 1, size=(len(pick), 1)).astype(np.int32)
            level = np.unique(np.concatenate([pick, nxt], axis=1), axis=0)
        counts.append(len(level))
        labels.append(level.reshape(-1))
        n_all += len(level)
    lab = np.ascontiguousarray(np.concatenate(labels), np.int32)
    p = np.round(rng.uniform(-4.0, -0.1, size=n_all), 4)
    b = np.round(rng.uniform(-1.0, 0.0, size=n_all), 4)
    h = ctypes.c_void_p()
    dp = ctypes.POINTER(ctypes.c_double)
    st = lib.pfhip_lm_graph_create(4, (ctypes.c_int * 4)(*counts), lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), p.ctypes.data_as(dp),
                                   b.ctypes.data_as(dp), V, 0.3, 0.1, -5.0, ctypes.byref(h))
    if st != 0:
        raise SystemExit(f"pfhip_lm_graph_create: status {st}: {lib.pfhip_last_error().decode()}")
    return h, n_all


def rows_of(rng, rows, k, V):
    ids = np.stack([rng.choice(V - 1, size=k, replace=False) + 1 for _ in range(rows)]).astype(np.int32)
    ids[rng.random(rows) < 0.4, 0] = 0                               # a CTC head's blank leads many rows
    lp = -np.cumsum(rng.uniform(0.05, 1.5, size=(rows, k)), axis=1).astype(np.float32)
    return ids, lp


def stats(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
            "stdev": round(statistics.pstdev(v), 4)}


def forwards(pkg, lib, have_lm, B, seconds, steps, warmup):
    """ms per batch of the two searching forwards, without and with the model: {name: {no_lm, lm}}."""
    import time
    weights = importlib.import_module("asr_2pass_amd.weights")
    rng = np.random.default_rng(20251114)                            # bench.py's audio
    n = seconds * 16000
    utts = []
    for i in range(B):
        t = np.arange(n, dtype=np.float64) / 16000.0
        x = 8000.0 * (0.6 * np.sin(2 * np.pi * 110.0 * 2.0 ** ((i % 24) / 12.0) * t) + 0.4 * rng.standard_normal(n))
        utts.append(np.clip(np.round(x), -32768, 32767).astype(np.int16))
    out = {}
    for name in ("sensevoice_forward_beam", "paraformer_forward_bias"):
        if name == "sensevoice_forward_beam":
            model = pkg.SenseVoiceHip().InitAsr(weights.synth_svs_weights(dict(weights.SENSEVOICE_SMALL)), device=0)
            V = int(model.cfg["vocab"])
            call = lambda: model.forward(utts, beam=(10, 10), nbest=1)
        else:
            model = pkg.ParaformerHip().InitAsr(weights.synth_weights(dict(weights.PARAFORMER_LARGE), seed=1234), device=0)
            V = model.vocab_size
            call = lambda: model.forward_bias(utts, [(8, 16, 1, None)])
        lm = pkg.LmGraph(synth_4gram(lib, V, 11)[0], V) if have_lm else None
        ms = {False: [], True: []}
        for k in range(warmup + steps):
            for w in ((False, True) if have_lm else (False,)):   # interleaved
                if have_lm:
                    model.set_token_lm(lm if w else None)
                t0 = time.perf_counter()
                call()
                if k >= warmup:
                    ms[w].append(1e3 * (time.perf_counter() - t0))
        out[name] = {"vocab": V, "no_lm": stats(ms[False])}
        if have_lm:
            out[name]["lm"] = stats(ms[True])
            out[name]["lm_minus_no_lm_median_ms"] = round(out[name]["lm"]["ms_median"] - out[name]["no_lm"]["ms_median"], 3)
        model.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", type=int, default=500)
    ap.add_argument("--seconds", type=int, default=30)
    ap.add_argument("--forward-steps", type=int, default=6)
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--no-model", action="store_true", help="the no-model series alone: what an older library runs, for the A/B")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    ops = importlib.import_module("asr_2pass_amd.ops")
    lib = pkg.load_lib()
    have_lm = hasattr(lib, "pfhip_op_nbest_ctx_beam_lm") and not args.no_model
    B, T = args.batch, args.rows
    rng = np.random.default_rng(7)
    off = torch.arange(B, dtype=torch.int32, device="cuda") * T
    n = torch.full((B,), T, dtype=torch.int32, device="cuda")
    searches = {}
    for name, V, k in (("ctc_prefix_beam", 25055, 10), ("nbest_ctx_beam", 8404, 8)):
        ids, lp = rows_of(rng, B * T, k, V)
        lm = None
        if have_lm:
            h, n_grams = synth_4gram(lib, V, 11)
            lm = pkg.LmGraph(h, V)
        searches[name] = dict(V=V, k=k, ids=torch.from_numpy(ids).cuda(), lp=torch.from_numpy(lp).cuda(), lm=lm,
                              n_grams=n_grams if have_lm else 0, image_mb=round(lib.pfhip_op_lm_score_workspace_bytes(lm.handle) / 2 ** 20, 1) if have_lm else 0)

    def launch(name, with_lm):
        s = searches[name]
        if name == "ctc_prefix_beam":
            a = (s["ids"], s["lp"], off, n, s["V"], [10] * B, [10] * B, [1] * B)
            return ops.ctc_prefix_beam_multi_lm(*a, s["lm"], max_tokens=T) if with_lm else ops.ctc_prefix_beam_multi(*a, max_tokens=T)
        a = (s["ids"], s["lp"], off, n, s["V"], [8] * B, [16] * B, [1] * B)
        return ops.nbest_ctx_beam_lm(*a, s["lm"], max_tokens=T) if with_lm else ops.nbest_ctx_beam(*a, max_tokens=T)

    def step(name, with_lm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = launch(name, with_lm)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    series = [(name, w) for name in searches for w in ((False, True) if have_lm else (False,))]
    for _ in range(max(args.warmup, 1)):
        for name, w in series:
            step(name, w)
    ms = {s: [] for s in series}
    last = {}
    for _ in range(max(args.steps, 1)):
        for s in series:                                             # interleaved
            t, last[s] = step(*s)
            ms[s].append(t)
    res = {"workload": f"{B} utterances x {T} candidate rows, one search launch", "steps": max(args.steps, 1), "warmup": max(args.warmup, 1)}
    for name in searches:
        r = {"vocab": searches[name]["V"], "columns": searches[name]["k"]}
        for w in ((False, True) if have_lm else (False,)):
            v = ms[(name, w)]
            r["lm" if w else "no_lm"] = stats(v)
        if have_lm:
            r["lm_ngrams"], r["lm_image_mb"] = searches[name]["n_grams"], searches[name]["image_mb"]
            r["lm_minus_no_lm_median_ms"] = round(r["lm"]["ms_median"] - r["no_lm"]["ms_median"], 4)
            a, b = last[(name, True)], last[(name, False)]
            r["best_changed_utterances"] = int(sum(not torch.equal(a[1][u, 0], b[1][u, 0]) for u in range(B)))
        res[name] = r
    if not args.no_forward:
        res["forward"] = dict(workload=f"{B} x {args.seconds} s synthetic 16 kHz, host buffers in, results out", steps=args.forward_steps,
                              **forwards(pkg, lib, have_lm, B, args.seconds, args.forward_steps, 2))
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
