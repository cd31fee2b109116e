"""CPU restatement of the DNSMOS speech-quality networks (the reference tree's utils/dnsmos_local.py with utils/DNSMOS/sig_bak_ovr.onnx
and model_v8.onnx), in torch / numpy, at float64 and float32.

Two forms of the same networks:
  * `primary_forward` / `p808_forward`: the networks written out by hand from the graphs — what the HIP kernels are compared with.
    They need only the initialisers, which lie under tests/golden/ as .npz under their ONNX names (`load_weights`);
  * `walk_graph`: an interpreter for the graphs' own nodes (Slice, Reshape, Concat, Transpose, Conv, Mul, Add, Sqrt, Pow, Max, Log, Div,
    Unsqueeze, Relu, MaxPool, ReduceMax, MatMul), run on a model read by asr_2pass_amd.onnx_reader.  Where the real files are present
    the tests hold the hand-written form against this walk, so the former is pinned by the files and not by memory.

What is NOT pinned by a file: `melspec`, the input of the P.808 net, which dnsmos_local.py:29-33 computes with librosa
(melspectrogram(n_fft = 321, hop_length = 160, n_mels = 120) then (power_to_db(S, ref = max) + 40) / 40).  librosa is not part of
this tree: its defaults — periodic Hann window, centred frames padded with ZEROS (the 0.10 default), Slaney mel scale with Slaney
normalisation over 0 .. sr / 2, power 2, amin 1e-10, top_db 80 — are RECALLED from librosa 0.10.0.

The clip loop (`extend_clip`, `clip_windows`, `polyfit`, `score_clip`) restates dnsmos_local.py:35-104, double arithmetic included."""
import glob
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FS = 16000
INPUT_LENGTH = 9.01
LEN_SAMPLES = int(INPUT_LENGTH * FS)          # 144160
N_FRAMES = 900
MEL_SAMPLES = LEN_SAMPLES - 160               # audio_seg[:-160]

# (Conv node, MaxPool behind its Relu) in graph order, and the three dense layers of the head
PRIMARY = dict(
    prefix="mos_estimator_logpow",
    convs=[("conv2d", False), ("conv2d_1", False), ("conv2d_2", False), ("conv2d_3", True), ("conv2d_4", True), ("conv2d_5", True),
           ("conv2d_6", False)],
    dense=["dense", "dense_1", "dense_3"])
P808 = dict(
    prefix="mos_estimator_small_1",
    convs=[("conv2d_5", True), ("conv2d_6", True), ("conv2d_7", False), ("conv2d_8", True), ("conv2d_9", False)],
    dense=["dense_3", "dense_4", "dense_5"])


def load_weights(kind):
    """The initialisers of the primary ("primary") or the P.808 ("p808") net from tests/golden/dnsmos_<kind>*.npz, by ONNX name."""
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, f"dnsmos_{kind}*.npz"))):
        with np.load(path) as z:
            for k in z.files:
                out[k] = z[k]
    if not out:
        raise FileNotFoundError(f"no tests/golden/dnsmos_{kind}*.npz")
    return out


def _t(a, dtype):
    return torch.as_tensor(np.array(a)).to(dtype)


# ---- the primary net's front end -----------------------------------------------------------------------------------------------------
def frames(x):
    """[N, 144160] -> [N, 900, 320]: Slice x 2, Reshape x 2, Concat on the last axis."""
    a = x[:, 0:144000].reshape(-1, N_FRAMES, 160)
    b = x[:, 160:144160].reshape(-1, N_FRAMES, 160)
    return torch.cat([a, b], dim=2)


def logpow(W, x, dtype=torch.float64):
    """input_1 [N, 144160] -> mos_estimator_logpow/truediv:0 [N, 900, 161]."""
    fr = frames(_t(x, dtype))
    wr = _t(W["time2freq/stft-real/kernel:0"], dtype)[:, :, 0]
    wi = _t(W["time2freq/stft-imag/kernel:0"], dtype)[:, :, 0]
    re, im = fr @ wr.T, fr @ wi.T
    mag = torch.sqrt(re * re + im * im)
    p = torch.pow(mag, _t(W["mos_estimator_logpow/pow/y:0"], dtype))
    p = torch.maximum(_t(W["mos_estimator_logpow/Maximum/x:0"], dtype), p)
    return torch.log(p) / _t(W["mos_estimator_logpow/truediv/y:0"], dtype)


# ---- the P.808 net's input (recalled librosa defaults: see the module docstring) -----------------------------------------------------
def _hz_to_mel(f):
    f = np.asarray(f, np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filters(sr=FS, n_fft=321, n_mels=120):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin = 0, fmax = sr / 2, htk = False, norm = 'slaney'): [n_mels, 1 + n_fft // 2], float64."""
    fftfreqs = np.arange(1 + n_fft // 2, dtype=np.float64) * sr / n_fft
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    w = np.zeros((n_mels, fftfreqs.size))
    for i in range(n_mels):
        w[i] = np.maximum(0.0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    return w * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]


def mel_power(audio, n_fft=321, hop=160, n_mels=120):
    """[MEL_SAMPLES] -> mel power [900, 120], float64."""
    y = np.asarray(audio, np.float64)
    y = np.pad(y, (n_fft // 2, n_fft // 2))
    k = np.arange(n_fft)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * k / n_fft)                    # scipy.signal.get_window("hann", n_fft, fftbins=True)
    n_fr = 1 + (y.size - n_fft) // hop
    idx = np.arange(n_fr)[:, None] * hop + k[None, :]
    spec = np.fft.rfft(y[idx] * win[None, :], axis=1)                   # [frames, 161]
    return (spec.real ** 2 + spec.imag ** 2) @ mel_filters(FS, n_fft, n_mels).T


def melspec(audio):
    """dnsmos_local.py's audio_melspec: (power_to_db(S, ref = max) + 40) / 40, transposed — [900, 120], float64."""
    S = mel_power(audio)
    amin, top_db = 1e-10, 80.0
    db = 10.0 * np.log10(np.maximum(amin, S)) - 10.0 * np.log10(np.maximum(amin, S.max()))
    db = np.maximum(db, db.max() - top_db)
    return (db + 40.0) / 40.0


# ---- the convolutions and the head ---------------------------------------------------------------------------------------------------
def conv_stack(W, net, h, dtype):
    """h [N, 1, H, W] (NCHW, as the graph has it) through Conv + Relu (+ MaxPool 2x2 / 2 VALID) groups."""
    for name, pool in net["convs"]:
        h = F.relu(F.conv2d(h, _t(W[f"{name}/kernel:0"], dtype), _t(W[f"{name}/bias:0"], dtype), stride=1, padding=1))
        if pool:
            h = F.max_pool2d(h, 2, 2)
    return h


def head(W, net, h, dtype):
    """ReduceMax over H and W, then MatMul + Add (+ Relu) three times."""
    v = h.amax(dim=(2, 3))
    for i, name in enumerate(net["dense"]):
        p = f"{net['prefix']}/{name}"
        v = v @ _t(W[f"{p}/MatMul/ReadVariableOp/resource:0"], dtype) + _t(W[f"{p}/BiasAdd/ReadVariableOp/resource:0"], dtype)
        if i < 2:
            v = F.relu(v)
    return v


def primary_forward(W, x, dtype=torch.float64):
    """[N, 144160] -> [N, 3] (sig, bak, ovr raw)."""
    h = logpow(W, x, dtype)[:, None, :, :]
    return head(W, PRIMARY, conv_stack(W, PRIMARY, h, dtype), dtype)


def p808_forward(W, mel, dtype=torch.float64):
    """[N, 900, 120] -> [N, 1]."""
    h = _t(mel, dtype)[:, None, :, :]
    return head(W, P808, conv_stack(W, P808, h, dtype), dtype)


# ---- the graphs' own nodes -----------------------------------------------------------------------------------------------------------
def walk_graph(model, feeds, dtype=torch.float64):
    """Runs an onnx_reader.OnnxModel node by node on torch tensors; float initialisers and feeds are taken at `dtype`.  Returns the
    dict of every value by name.  Raises NotImplementedError at the first node outside the DNSMOS graphs' operator set."""
    env = {}
    for k, v in model.initializers.items():
        env[k] = _t(v, dtype) if np.issubdtype(np.asarray(v).dtype, np.floating) else torch.as_tensor(np.array(v))
    for k, v in feeds.items():
        env[k] = _t(v, dtype)
    for nd in model.nodes:
        i = [env[n] for n in nd.inputs]
        a, op = nd.attrs, nd.op_type
        if op == "Slice":
            t, st, en, ax, sp = i[0], *(v.tolist() for v in i[1:5])
            for s0, e0, d, s1 in zip(st, en, ax, sp):
                n = t.shape[d]
                if s0 < 0 or e0 < 0 or s1 < 1:
                    raise NotImplementedError(f"Slice {nd.name}: negative bounds")
                sl = [slice(None)] * t.dim()
                sl[d] = slice(min(s0, n), min(e0, n), s1)
                t = t[tuple(sl)]
            y = t
        elif op == "Reshape":
            y = i[0].reshape([int(v) for v in i[1].tolist()])
        elif op == "Concat":
            y = torch.cat(i, dim=int(a["axis"]))
        elif op == "Transpose":
            y = i[0].permute(*[int(v) for v in a["perm"]])
        elif op == "Conv":
            ks = list(a["kernel_shape"])
            pads = list(a.get("pads", [0] * (2 * len(ks))))
            if a.get("auto_pad", "NOTSET") not in ("NOTSET", "VALID", b"NOTSET", b"VALID") or pads[:len(ks)] != pads[len(ks):]:
                raise NotImplementedError(f"Conv {nd.name}: padding")
            bias = i[2] if len(i) > 2 else None
            fn = F.conv1d if len(ks) == 1 else F.conv2d
            y = fn(i[0], i[1], bias, stride=list(a["strides"]), padding=pads[:len(ks)], dilation=list(a["dilations"]), groups=int(a["group"]))
        elif op == "MaxPool":
            if int(a.get("ceil_mode", 0)) or any(a.get("pads", [0])):
                raise NotImplementedError(f"MaxPool {nd.name}")
            y = F.max_pool2d(i[0], list(a["kernel_shape"]), list(a["strides"]))
        elif op == "ReduceMax":
            y = i[0].amax(dim=[int(v) for v in a["axes"]], keepdim=bool(a.get("keepdims", 1)))
        elif op == "Unsqueeze":
            y = i[0]
            for d in a["axes"]:
                y = y.unsqueeze(int(d))
        elif op in ("Mul", "Add", "Div", "Pow", "Max", "MatMul"):
            y = {"Mul": torch.mul, "Add": torch.add, "Div": torch.div, "Pow": torch.pow, "Max": torch.maximum, "MatMul": torch.matmul}[op](*i)
        elif op in ("Sqrt", "Log", "Relu"):
            y = {"Sqrt": torch.sqrt, "Log": torch.log, "Relu": F.relu}[op](i[0])
        else:
            raise NotImplementedError(f"{op} ({nd.name})")
        env[nd.outputs[0]] = y
    return env


# ---- the clip loop (dnsmos_local.py:51-104) ------------------------------------------------------------------------------------------
def extend_clip(audio):
    """A clip shorter than 144160 samples is appended to itself until it is not."""
    audio = np.asarray(audio)
    while len(audio) < LEN_SAMPLES:
        audio = np.append(audio, audio)
    return audio


def clip_windows(n_samples):
    """(num_hops, [(begin, end) of the windows that are scored]) of an (already extended) clip of n_samples samples.  The bounds are
    the reference's own double arithmetic: for some idx the end falls one sample short, and that window is skipped."""
    num_hops = int(np.floor(n_samples / FS) - INPUT_LENGTH) + 1
    kept = []
    for idx in range(num_hops):
        b, e = int(idx * FS), int((idx + INPUT_LENGTH) * FS)
        if min(e, n_samples) - min(b, n_samples) < LEN_SAMPLES:
            continue
        kept.append((b, e))
    return num_hops, kept


POLY = {
    False: dict(ovr=[-0.06766283, 1.11546468, 0.04602535], sig=[-0.08397278, 1.22083953, 0.0052439],
                bak=[-0.13166888, 1.60915514, -0.39604546]),
    True: dict(ovr=[-0.00533021, 0.005101, 1.18058466, -0.11236046], sig=[-0.01019296, 0.02751166, 1.19576786, -0.24348726],
               bak=[-0.04976499, 0.44276479, -0.1644611, 0.96883132]),
}


def polyfit(sig, bak, ovr, personalized):
    """get_polyfit_val: np.poly1d (highest power first), in double."""
    c = POLY[bool(personalized)]
    return tuple(float(np.polyval(np.asarray(c[k], np.float64), np.float64(v))) for k, v in (("sig", sig), ("bak", bak), ("ovr", ovr)))


def score_clip(raw, num_hops, personalized=False):
    """raw [n_scored, 4] = (p808, sig, bak, ovr) per scored window -> the clip's result: counts, and means in double."""
    raw = np.asarray(raw, np.float64).reshape(-1, 4)
    fit = np.array([polyfit(r[1], r[2], r[3], personalized) for r in raw]).reshape(-1, 3)
    mean = lambda v: float(np.mean(v)) if len(v) else float("nan")
    return dict(num_hops=int(num_hops), n_scored=int(raw.shape[0]), p808=mean(raw[:, 0]), sig_raw=mean(raw[:, 1]), bak_raw=mean(raw[:, 2]),
                ovr_raw=mean(raw[:, 3]), sig=mean(fit[:, 0]), bak=mean(fit[:, 1]), ovr=mean(fit[:, 2]))


# ---- the golden cases: inputs from seeds --------------------------------------------------------------------------------------------
CASES = ("tone_noise", "zeros", "clipped_square")


def case_window(name):
    """One 144160-sample window, float32 in [-1, 1], every value k / 32768 so that the 16-bit form of the same window is exact."""
    n = LEN_SAMPLES
    t = np.arange(n, dtype=np.float64) / FS
    if name == "tone_noise":
        rng = np.random.default_rng(20261020)
        x = 8000.0 * (0.6 * np.sin(2 * np.pi * 220.0 * t) + 0.4 * rng.standard_normal(n))
    elif name == "zeros":
        x = np.zeros(n)
    elif name == "clipped_square":
        x = 60000.0 * np.sign(np.sin(2 * np.pi * 440.0 * t + 0.1))
    else:
        raise KeyError(name)
    return (np.clip(np.round(x), -32768, 32767) / 32768.0).astype(np.float32)
