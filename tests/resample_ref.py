"""NumPy restatement of the resampling the reference runs ahead of its front end (test helper).

Audio::WavResample (onnxruntime/src/audio.cpp:259-284) builds a fresh Kaldi LinearResample (onnxruntime/src/resample.cpp) with
cutoff 0.99 * 0.5 * min(fs_in, fs_out) and 6 zero crossings, and resamples the whole buffer with flush = true.  The precision
choices are the reference's: the cutoff is a float; the filter function takes a float t and evaluates window and sinc in double
through libm (math.cos / math.sin here), rounds each to float and returns their float product; each weight is that product
divided by the input rate in float.  Each output is the serial float32 sum over the taps in order, acc = acc + w[j] * x[idx],
with taps outside [0, n) skipped.
"""
from __future__ import annotations

import math

import numpy as np

ZEROS = 6
MIN_RATE, MAX_RATE = 1000, 192000
TWO_PI = 6.283185307179586476925286766559005
PI = 3.1415926535897932384626433832795
f32 = np.float32


def supported(fs_in: int, fs_out: int) -> bool:
    if not (MIN_RATE <= fs_in <= MAX_RATE and MIN_RATE <= fs_out <= MAX_RATE):
        return False
    return fs_in // math.gcd(fs_in, fs_out) * fs_out <= 2**31 - 1


def out_len(fs_in: int, fs_out: int, n: int) -> int:
    """LinearResample::GetNumOutputSamples with flush (resample.cpp:220-265); -1 for an unsupported pair."""
    if not supported(fs_in, fs_out) or n < 0:
        return -1
    if fs_in == fs_out:
        return n
    tick = fs_in // math.gcd(fs_in, fs_out) * fs_out
    interval = n * (tick // fs_in)
    if interval <= 0:
        return 0
    per_out = tick // fs_out
    last = interval // per_out
    if last * per_out == interval:
        last -= 1
    return last + 1


def cutoff(fs_in: int, fs_out: int) -> np.float32:
    return f32(0.99 * 0.5 * float(f32(min(fs_in, fs_out))))


def _filter(t: np.float32, fc: np.float32) -> np.float32:
    td, fcd = float(t), float(fc)
    if abs(td) < ZEROS / (2.0 * fcd):
        window = f32(0.5 * (1 + math.cos(TWO_PI * fcd / ZEROS * td)))
    else:
        window = f32(0.0)
    if td != 0:
        filt = f32(math.sin(TWO_PI * fcd * td) / (PI * td))
    else:
        filt = f32(2) * fc
    return f32(filt * window)


def plan(fs_in: int, fs_out: int):
    """SetIndexesAndWeights (resample.cpp:104-136) -> (P, first_index int32 [Q], ntaps int32 [Q], weights float32 [Q, K])."""
    base = math.gcd(fs_in, fs_out)
    P, Q = fs_in // base, fs_out // base
    fc = cutoff(fs_in, fs_out)
    width = ZEROS / (2.0 * float(fc))
    first = np.zeros(Q, np.int32)
    ntaps = np.zeros(Q, np.int32)
    rows = []
    for i in range(Q):
        out_t = i / float(fs_out)
        lo = math.ceil((out_t - width) * fs_in)
        hi = math.floor((out_t + width) * fs_in)
        first[i], ntaps[i] = lo, hi - lo + 1
        rows.append([f32(_filter(f32((lo + j) / float(fs_in) - out_t), fc) / f32(fs_in)) for j in range(hi - lo + 1)])
    K = int(ntaps.max())
    w = np.zeros((Q, K), np.float32)
    for i, r in enumerate(rows):
        w[i, :len(r)] = r
    return P, first, ntaps, w


_PLANS: dict = {}


def cached_plan(fs_in: int, fs_out: int):
    key = (fs_in, fs_out)
    if key not in _PLANS:
        _PLANS[key] = plan(fs_in, fs_out)
    return _PLANS[key]


def resample(x: np.ndarray, fs_in: int, fs_out: int = 16000) -> np.ndarray:
    """Audio::WavResample on float32 samples x (a bitwise copy when the rates are equal)."""
    x = np.ascontiguousarray(x, np.float32)
    if fs_in == fs_out:
        return x.copy()
    n = x.shape[0]
    n_out = out_len(fs_in, fs_out, n)
    if n_out < 0:
        raise ValueError(f"unsupported rate pair {fs_in} -> {fs_out}")
    P, first, ntaps, w = cached_plan(fs_in, fs_out)
    Q, K = w.shape
    s = np.arange(n_out, dtype=np.int64)
    ph = s % Q
    f = first[ph].astype(np.int64) + (s // Q) * P
    nt = ntaps[ph]
    acc = np.zeros(n_out, np.float32)
    xp = x if n else np.zeros(1, np.float32)
    for j in range(K):
        idx = f + j
        ok = (j < nt) & (idx >= 0) & (idx < n)
        v = xp[np.clip(idx, 0, max(n - 1, 0))]
        acc = np.where(ok, acc + w[ph, j] * v, acc).astype(np.float32)
    return acc
