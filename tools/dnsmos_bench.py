"""DnsMosHip timing: ms per 9.01-s window at N = 1, 8, 64 windows in a call and on a 10-minute clip (570 scored windows), the achieved
TFLOP/s of the convolutions (38.63 GFLOP per window in the primary net, 0.87 in the P.808 net) against the 833-TFLOP/s roof of the
three-product fp16 form, and beside it the float32 CPU restatement (tests/dnsmos_ref.py, torch on 16 threads) as the stated baseline.

    python tools/dnsmos_bench.py [--model-dir /path/to/utils] [--reps 3]

Without --model-dir the weights come from tests/golden/ (written out as .onnx files into a temporary directory)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GFLOP_PRIMARY, GFLOP_P808, ROOF_TF = 38.63, 0.87, 833.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-windows", type=int, default=2)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    import dnsmos_onnx as O
    import dnsmos_ref as R
    pkg = ge.load_package()
    if a.model_dir:
        primary, p808 = os.path.join(a.model_dir, "DNSMOS/sig_bak_ovr.onnx"), os.path.join(a.model_dir, "DNSMOS/model_v8.onnx")
    else:
        d = tempfile.mkdtemp()
        primary, p808 = os.path.join(d, "sig_bak_ovr.onnx"), os.path.join(d, "model_v8.onnx")
        open(primary, "wb").write(O.primary_onnx(R.load_weights("primary")))
        open(p808, "wb").write(O.p808_onnx(R.load_weights("p808")))
    mos = pkg.DnsMosHip().InitMos(primary, p808)
    rng = np.random.default_rng(1)
    res = {}

    def timed(clips):
        mos.score_windows(clips)                                  # warm-up
        best = float("inf")
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, scored, _ = mos.score_windows(clips)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        return best, sum(scored)

    for n in (1, 8, 64):
        clips = [(rng.standard_normal(R.LEN_SAMPLES) * 0.1).astype(np.float32) for _ in range(n)]
        t, k = timed(clips)
        res[f"N={n}"] = dict(windows=k, ms_per_window=1e3 * t / k, conv_tflops=k * (GFLOP_PRIMARY + GFLOP_P808) / t / 1e3)
    t, k = timed([(rng.standard_normal(600 * 16000) * 0.1).astype(np.float32)])
    res["10min"] = dict(windows=k, ms_per_window=1e3 * t / k, conv_tflops=k * (GFLOP_PRIMARY + GFLOP_P808) / t / 1e3, seconds=t)
    for v in res.values():
        v["of_roof"] = v["conv_tflops"] / ROOF_TF
    # the stated baseline: the float32 restatement on the CPU
    torch.set_num_threads(16)
    Wp, W8 = R.load_weights("primary"), R.load_weights("p808")
    x = np.stack([(rng.standard_normal(R.LEN_SAMPLES) * 0.1).astype(np.float32) for _ in range(a.cpu_windows)])
    mel = np.stack([R.melspec(w[:R.MEL_SAMPLES]) for w in x]).astype(np.float32)
    with torch.no_grad():
        R.primary_forward(Wp, x[:1], torch.float32)
        t0 = time.perf_counter()
        R.primary_forward(Wp, x, torch.float32)
        R.p808_forward(W8, mel, torch.float32)
        res["cpu_f32_16_threads"] = dict(ms_per_window=1e3 * (time.perf_counter() - t0) / len(x))
    mos.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
