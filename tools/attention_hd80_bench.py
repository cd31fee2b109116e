"""Dev tool (GPU): the d_k = 80 attention (attention_h80.hip) against attention_x3.hip (d_k = 128) at the same launch shape, and the
small Paraformer end to end.

  python tools/attention_hd80_bench.py kernel    B = 32 utterances x T = 500 rows x H = 4 heads, self-attention, both widths from one
                                                 build in one process, alternated in rounds; device events over `reps` launches each
                                                 (launch gaps included: back-to-back launches on one stream), best and median round
  python tools/attention_hd80_bench.py offline   the small model (PARAFORMER_SMALL, random-init) on 32 x 30 s: audio-seconds per second
  python tools/attention_hd80_bench.py stream    one connection, 600-ms chunks: ms per chunk (host clock around the synchronous call)
  (no argument: all three).  Run each mode under its own `timeout -k`, chained with `&&`."""
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
wt = importlib.import_module(pkg.__name__ + ".weights")
ops = importlib.import_module(pkg.__name__ + ".ops")
from conftest import synth_pcm  # noqa: E402

B, T, H = 32, 500, 4


def bench_kernel(reps=200, rounds=7):
    rng = np.random.default_rng(1)
    off = torch.from_numpy((np.arange(B) * T).astype(np.int32)).cuda()
    ln = torch.from_numpy(np.full(B, T, np.int32)).cuda()
    ops_in = {}
    for dk in (80, 128):
        q, k, v = (torch.from_numpy(rng.standard_normal((B * T, H * dk)).astype(np.float32)).cuda() for _ in range(3))
        ops_in[dk] = (q, k, v)
        for _ in range(3):                                        # warm-up: code object, LDS opt-in
            ops.attention(q, k, v, off, ln, off, ln, H, dk ** -0.5, head_dim=dk)
    torch.cuda.synchronize()
    us = {80: [], 128: []}
    for _ in range(rounds):
        for dk in (80, 128):                                      # alternated: both see the same neighbours on the machine
            q, k, v = ops_in[dk]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ops.attention(q, k, v, off, ln, off, ln, H, dk ** -0.5, head_dim=dk)
            e1.record()
            torch.cuda.synchronize()
            us[dk].append(e0.elapsed_time(e1) * 1e3 / reps)
    for dk in (80, 128):
        flops = 4.0 * B * H * T * T * dk
        best, med = min(us[dk]), statistics.median(us[dk])
        print(json.dumps({"mode": "kernel", "d_k": dk, "B": B, "T": T, "H": H, "us_best": round(best, 2), "us_median": round(med, 2),
                          "us_rounds": [round(x, 2) for x in us[dk]], "GFLOP": round(flops / 1e9, 3),
                          "TFLOPs_at_median": round(flops / med / 1e6, 1)}), flush=True)
    print(json.dumps({"mode": "kernel", "ratio_80_over_128_median": round(statistics.median(us[80]) / statistics.median(us[128]), 3),
                      "flop_ratio": 0.625}), flush=True)


def small_model():
    man, blob = wt.synth_weights(dict(wt.PARAFORMER_SMALL), seed=1)
    return pkg.ParaformerHip().InitAsr((man, blob))


def bench_offline(steps=8, warmup=2):
    model = small_model()
    rng = np.random.default_rng(2)
    utts = [synth_pcm(i, 16000 * 30, rng) for i in range(32)]
    for _ in range(warmup):
        model.forward_ids(utts)
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        model.forward_ids(utts)
        ts.append(time.perf_counter() - t0)
    med = statistics.median(ts)
    print(json.dumps({"mode": "offline", "model": "PARAFORMER_SMALL (random init)", "batch": 32, "secs": 30, "ms_per_step_median": round(med * 1e3, 2),
                      "ms_best": round(min(ts) * 1e3, 2), "audio_s_per_s": round(32 * 30 / med, 1),
                      "note": "host call incl. PCM upload and result fetch"}), flush=True)
    model.close()


def bench_stream(chunks=60, warmup=10):
    model = small_model()
    rng = np.random.default_rng(3)
    pcm = synth_pcm(5, 9600 * (chunks + warmup), rng)
    st = pkg.ParaformerOnlineHip(model)
    ts = []
    for j in range(chunks + warmup):
        t0 = time.perf_counter()
        st.Forward(pcm[j * 9600:(j + 1) * 9600], input_finished=False)
        if j >= warmup:
            ts.append(time.perf_counter() - t0)
    print(json.dumps({"mode": "stream", "model": "PARAFORMER_SMALL (random init)", "chunk_ms": 600, "ms_per_chunk_median": round(statistics.median(ts) * 1e3, 3),
                      "ms_p90": round(sorted(ts)[int(0.9 * len(ts))] * 1e3, 3), "chunks": chunks}), flush=True)
    st.close()
    model.close()


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("needs a GPU: nothing here is measured on a CPU")
    modes = sys.argv[1:] or ["kernel", "offline", "stream"]
    for m in modes:
        {"kernel": bench_kernel, "offline": bench_offline, "stream": bench_stream}[m]()
