"""Dev tool (GPU): the resampling ahead of the front end.

  python tools/resample_bench.py kernel   the kernel alone (pfhip_op_resample) on 32 x 30 s at 8 / 44.1 / 48 kHz: us and GB/s
  python tools/resample_bench.py forward  pfhip_offline_forward_rate at 8 kHz against pfhip_offline_forward at 16 kHz, same audio
                                          (32 x 30 s, Paraformer-large-sized random-init weights)
  python tools/resample_bench.py tpass    2-pass per-call p50 / p99 through `tpass_bench` with 48 kHz messages against 16 kHz
  (no argument: all three).  Run under `timeout -k`; for kernel figures that do not include launch gaps, wrap the `kernel` mode in
  `rocprofv3 --kernel-trace --stats -- python tools/resample_bench.py kernel`."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
import importlib  # noqa: E402

wt = importlib.import_module(pkg.__name__ + ".weights")
ops = importlib.import_module(pkg.__name__ + ".ops")
from conftest import synth_pcm  # noqa: E402

B, SECS = 32, 30


def audio(fs, rng, n_utt=B, secs=SECS):
    return [(np.clip(np.round(8000 * rng.standard_normal(fs * secs)), -32768, 32767) / 32768.0).astype(np.float32)
            for _ in range(n_utt)]


def bench_kernel(reps=50):
    rng = np.random.default_rng(1)
    for fs in (8000, 44100, 48000):
        utts = audio(fs, rng)
        offs = np.cumsum([0] + [len(u) for u in utts[:-1]])
        x = torch.from_numpy(np.concatenate(utts)).cuda()
        lens = [len(u) for u in utts]
        y, _, n_out = ops.resample(x, offs, lens, fs)           # warm-up: plan upload, code object
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ops.resample(x, offs, lens, fs)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps
        nbytes = 4 * (sum(lens) + sum(n_out))
        print(json.dumps({"mode": "kernel", "fs_in": fs, "batch": B, "secs": SECS, "in_MB": round(4 * sum(lens) / 1e6, 1),
                          "out_MB": round(4 * sum(n_out) / 1e6, 1), "us_per_call_incl_launch": round(us, 1),
                          "GB_s": round(nbytes / us / 1e3, 1)}), flush=True)


def bench_forward(reps=5):
    man, blob = wt.synth_weights(dict(wt.PARAFORMER_LARGE), seed=1234)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    rng = np.random.default_rng(2)
    a8 = audio(8000, rng)
    a16 = m.resample(a8, 8000)                                  # the same audio at the model's rate
    res = {}
    for name, din, rate in (("forward_16k", a16, None), ("forward_rate_8k", a8, 8000)):
        m.forward_ids(din, sample_rate=rate)
        t0 = time.perf_counter()
        for _ in range(reps):
            r = m.forward_ids(din, sample_rate=rate)
        res[name] = (time.perf_counter() - t0) / reps * 1e3
        res[name + "_ids"] = [list(map(int, x)) for x in r["ids"]]
    same = res["forward_16k_ids"] == res["forward_rate_8k_ids"]
    print(json.dumps({"mode": "forward", "batch": B, "secs": SECS, "forward_16k_ms": round(res["forward_16k"], 2),
                      "forward_rate_8k_ms": round(res["forward_rate_8k"], 2), "same_ids": same}), flush=True)
    m.close()


def bench_tpass(seconds=20, conns=16):
    from test_gpu_pipeline import shape_vad_weights
    d = tempfile.mkdtemp(prefix="resample_tpass_")
    cfg = dict(wt.PARAFORMER_LARGE)
    for name, seed in (("asr", 31), ("online", 32)):
        os.mkdir(os.path.join(d, name))
        man, blob = wt.synth_weights(cfg, seed=seed)
        wt.save(os.path.join(d, name, "model.pfhip"), man, blob)
    os.mkdir(os.path.join(d, "vad"))
    vman, vblob = shape_vad_weights(*wt.synth_vad_weights())
    wt.save(os.path.join(d, "vad", "vad.pfhip"), vman, vblob)
    exe = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "tpass_bench")
    for fs in (16000, 48000):
        rng = np.random.default_rng(5)
        parts, total, i = [], 0, 0
        while total < seconds * fs:
            sec = [4.0, 7.5, 2.2, 11.0, 5.3][i % 5]
            parts += [synth_pcm(i, int(sec * fs), rng), np.zeros(int(1.2 * fs), np.float32)]
            total += len(parts[-2]) + len(parts[-1])
            i += 1
        pcm = np.concatenate(parts)[:seconds * fs]
        f = os.path.join(d, f"stream_{fs}.pcm")
        np.clip(np.round(pcm * 32768.0), -32768, 32767).astype("<i2").tofile(f)
        out = subprocess.run([exe, os.path.join(d, "asr"), os.path.join(d, "online"), os.path.join(d, "vad"), "-", f, str(conns), "2",
                              str(fs)], capture_output=True, text=True, timeout=400)
        print(json.dumps({"mode": "tpass", "audio_fs": fs}), out.stdout.strip() or out.stderr[-2000:], flush=True)
        if out.returncode != 0:
            raise SystemExit(out.returncode)
    import shutil
    shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what in ("kernel", "all"):
        bench_kernel()
    if what in ("forward", "all"):
        bench_forward()
    if what in ("tpass", "all"):
        bench_tpass()
