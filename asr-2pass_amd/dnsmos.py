"""DnsMosHip: clip-level speech-quality scores (the reference tree's utils/dnsmos_local.py) through the C ABI's pfhip_mos_* family
(include/pfhip.h, csrc/mos.cpp), and the Python twin of the C++ reader of the two .onnx files (csrc/mos_files.cpp): `read_family`
walks a graph exactly as the C++ walk does and `container` lays the same "dnsmos" container out, bit for bit.

Audio is 16 kHz; other rates go through pfhip_resample first, which is Kaldi's LinearResample — NOT librosa.resample, which the
reference script calls: scores of resampled audio differ from the script's by that much.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import PfhipError, _check, load_lib, onnx_reader

FS = 16000
INPUT_LENGTH = 9.01
LEN_SAMPLES = int(INPUT_LENGTH * FS)      # 144160
ALIGN = 256
_FRONT = ["Slice", "Slice", "Reshape", "Reshape", "Concat", "Conv", "Conv", "Mul", "Mul", "Add", "Sqrt", "Pow", "Max", "Log", "Div"]


def _plain_auto_pad(a):
    v = a.get("auto_pad", "NOTSET")
    return (v.decode() if isinstance(v, bytes) else v) in ("NOTSET", "VALID")


def read_family(path_or_model, primary):
    """The skeleton of a DNSMOS graph, by the rules of csrc/mos_files.cpp (see its head): dict(front = None | [wr, wi, consts],
    convs = [(w, b, pool)], dense = [(w, b)]).  Raises PfhipError naming the first node that does not fit."""
    m = path_or_model if isinstance(path_or_model, onnx_reader.OnnxModel) else onnx_reader.read_model(path_or_model)
    init = {k: v for k, v in m.initializers.items() if k not in m.external}

    def refuse(nd, why):
        raise PfhipError(f"not a DNSMOS graph: node {nd.name or (nd.outputs[0] if nd.outputs else '?')} ({nd.op_type}): {why}")

    def f32(name):
        a = init.get(name)
        return a if a is not None and a.dtype == np.float32 else None

    n_front = len(_FRONT) if primary else 0
    at, stft, consts = 0, {}, [0.0, 0.0, 0.0]
    convs, dense, stage = [], [], 0
    last_conv_out = last_relu_out = last_relu_src = dense_out = None
    pooled = have_max = False
    for nd in m.nodes:
        op, a = nd.op_type, nd.attrs
        if at < n_front:
            if op in ("Transpose", "Unsqueeze"):
                continue
            if op != _FRONT[at]:
                refuse(nd, f"the front end needs a {_FRONT[at]} here")
            if op == "Conv":
                w = f32(nd.inputs[1]) if len(nd.inputs) == 2 else None
                if w is None:
                    refuse(nd, "the STFT kernel is not an initialiser of the file")
                real, imag = "stft-real" in nd.inputs[1], "stft-imag" in nd.inputs[1]
                if real == imag or ("wr" if real else "wi") in stft:
                    refuse(nd, f"its kernel {nd.inputs[1]} is not named as the real or the imaginary STFT kernel")
                if (w.shape != (161, 320, 1) or list(a.get("kernel_shape", [])) != [1] or list(a.get("strides", [])) != [1]
                        or int(a.get("group", 1)) != 1 or not _plain_auto_pad(a)):
                    refuse(nd, "not a [161, 320, 1] float kernel applied as a 1x1 convolution")
                stft["wr" if real else "wi"] = w
            elif op in ("Pow", "Max", "Div"):
                c = [init[n] for n in nd.inputs if n in init]
                if len(c) != 1 or c[0].size != 1 or c[0].dtype != np.float32:
                    refuse(nd, "its constant is not one scalar float initialiser")
                consts[{"Max": 0, "Pow": 1, "Div": 2}[op]] = c[0].reshape(-1)[0]
            at += 1
            continue
        if op in ("Transpose", "Unsqueeze"):
            continue
        if op == "Conv" and stage == 0:
            w = f32(nd.inputs[1]) if len(nd.inputs) == 3 else None
            b = f32(nd.inputs[2]) if len(nd.inputs) == 3 else None
            if w is None:
                refuse(nd, "its kernel is not an initialiser of the file")
            if b is None:
                refuse(nd, "its bias is not an initialiser of the file")
            dil = list(a.get("dilations", []))
            if (w.ndim != 4 or w.shape[2:] != (3, 3) or not 1 <= w.shape[0] <= 4096 or not 1 <= w.shape[1] <= 4096 or b.shape != (w.shape[0],)
                    or list(a.get("pads", [])) != [1, 1, 1, 1] or list(a.get("strides", [])) != [1, 1] or (dil and dil != [1, 1])
                    or int(a.get("group", 1)) != 1 or not _plain_auto_pad(a)):
                refuse(nd, "not a 3x3 / pads 1 / strides 1 float convolution with a bias")
            if w.shape[1] != (convs[-1][0].shape[0] if convs else 1):
                refuse(nd, "its input channels do not follow from the layer before")
            convs.append([w, b, False])
            last_conv_out, pooled = (nd.outputs[0] if nd.outputs else ""), False
        elif op == "Relu":
            if len(nd.inputs) != 1 or not nd.outputs:
                refuse(nd, "malformed")
            if (nd.inputs[0] != last_conv_out) if stage == 0 else (nd.inputs[0] != dense_out or not dense or dense[-1][1] is None):
                refuse(nd, "a Relu that does not follow a convolution or a dense layer")
            last_relu_out, last_relu_src = nd.outputs[0], nd.inputs[0]
            if stage == 1:
                dense_out = nd.outputs[0]
        elif op == "MaxPool" and stage == 0:
            if (len(nd.inputs) != 1 or nd.inputs[0] != last_relu_out or last_relu_src != last_conv_out or pooled or not convs
                    or list(a.get("kernel_shape", [])) != [2, 2] or list(a.get("strides", [])) != [2, 2] or any(a.get("pads", []))
                    or int(a.get("ceil_mode", 0)) or not _plain_auto_pad(a)):
                refuse(nd, "not a 2x2 / strides 2 floor pool directly behind a convolution's Relu")
            convs[-1][2], pooled = True, True
            last_relu_out = nd.outputs[0] if nd.outputs else ""
        elif op == "ReduceMax" and stage == 0 and convs:
            if list(a.get("axes", [])) != [1, 2] or int(a.get("keepdims", 1)) != 0:
                refuse(nd, "not a maximum over axes 1 and 2")
            stage, have_max = 1, True
            dense_out = nd.outputs[0] if nd.outputs else ""
        elif op == "MatMul" and stage == 1:
            w = f32(nd.inputs[1]) if len(nd.inputs) == 2 else None
            if w is None or nd.inputs[0] != dense_out or w.ndim != 2 or not 1 <= w.shape[0] <= 256 or not 1 <= w.shape[1] <= 256:
                refuse(nd, "not a dense layer (at most 256 wide) on the value before it, with its float weight in the file")
            if w.shape[0] != (dense[-1][0].shape[1] if dense else convs[-1][0].shape[0]):
                refuse(nd, "its input width does not follow from the layer before")
            if dense and dense[-1][1] is None:
                refuse(nd, "the dense layer before it has no bias")
            dense.append([w, None])
            dense_out = nd.outputs[0] if nd.outputs else ""
        elif op == "Add" and stage == 1 and dense and dense[-1][1] is None:
            other = [n for n in nd.inputs if n != dense_out]
            b = f32(other[0]) if len(nd.inputs) == 2 and len(other) == 1 else None
            if b is None or b.shape != (dense[-1][0].shape[1],):
                refuse(nd, "not the bias of the dense layer before it")
            dense[-1][1] = b
            dense_out = nd.outputs[0] if nd.outputs else ""
        else:
            refuse(nd, "an operator outside the family, or out of place")
    if at < n_front:
        raise PfhipError(f"not a DNSMOS primary graph: the front end ends before its {_FRONT[at]}")
    if not have_max or len(dense) != 3 or dense[-1][1] is None:
        raise PfhipError("not a DNSMOS graph: it needs convolutions, a global maximum and three dense layers with biases")
    if dense[-1][0].shape[1] != (3 if primary else 1):
        raise PfhipError("not a DNSMOS primary graph: the head must have three outputs" if primary else
                         "not a DNSMOS P.808 graph: the head must have one output")
    front = [stft["wr"][:, :, 0], stft["wi"][:, :, 0], np.array(consts, np.float32)] if primary else None
    return dict(front=front, convs=[tuple(c) for c in convs], dense=[tuple(d) for d in dense])


def container(primary, p808=None):
    """(manifest dict, float32 blob) of kind "dnsmos" from the two .onnx files (paths or OnnxModel objects): the bytes
    pfhip_read_model_files("dnsmos", ...) gives."""
    nets = [("primary", read_family(primary, True))] + ([("p808", read_family(p808, False))] if p808 is not None else [])
    tensors, parts, off = {}, [], 0

    def put(name, arr, shape):
        nonlocal off
        a = np.ascontiguousarray(arr, np.float32).reshape(-1)
        tensors[name] = {"shape": [int(v) for v in shape], "offset": off}
        padded = (a.size * 4 + ALIGN - 1) // ALIGN * ALIGN
        buf = np.zeros(padded // 4, np.float32)
        buf[:a.size] = a
        parts.append(buf)
        off += padded

    cfg = {"kind": "dnsmos", "has_p808": 1 if p808 is not None else 0, "primary_convs": [], "primary_dense": [], "p808_convs": [], "p808_dense": []}
    for pre, fam in nets:
        if fam["front"]:
            put(f"{pre}.stft_real", fam["front"][0], (161, 320))
            put(f"{pre}.stft_imag", fam["front"][1], (161, 320))
            put(f"{pre}.consts", fam["front"][2], (3,))
        for i, (w, b, pool) in enumerate(fam["convs"]):
            put(f"{pre}.conv{i}.w", w, w.shape)
            put(f"{pre}.conv{i}.b", b, b.shape)
            cfg[f"{pre}_convs"] += [int(w.shape[0]), int(w.shape[1]), 1 if pool else 0]
        for i, (w, b) in enumerate(fam["dense"]):
            put(f"{pre}.dense{i}.w", w, w.shape)
            put(f"{pre}.dense{i}.b", b, b.shape)
            cfg[f"{pre}_dense"] += [int(w.shape[0]), int(w.shape[1])]
    return {"config": cfg, "tensors": tensors, "total_bytes": off}, np.concatenate(parts)


class _Result(ctypes.Structure):
    _fields_ = [("num_hops", ctypes.c_int32), ("n_scored", ctypes.c_int32)] + [(k, ctypes.c_double) for k in
                                                                              ("p808", "sig_raw", "bak_raw", "ovr_raw", "sig", "bak", "ovr")]


def windows_of(n_samples):
    """(extended length, num_hops, windows scored) of a clip of n_samples samples, by the clip loop's own arithmetic — what a caller
    sizes pfhip_mos_score_windows' buffer with."""
    n = int(n_samples)
    if n < 1:
        raise PfhipError("an empty clip has no score")
    while n < LEN_SAMPLES:
        n *= 2
    hops = int(math.floor(n / FS) - INPUT_LENGTH) + 1
    kept = sum(1 for i in range(hops) if min(int((i + INPUT_LENGTH) * FS), n) - min(int(i * FS), n) >= LEN_SAMPLES)
    return n, hops, kept


class DnsMosHip:
    def __init__(self):
        self._lib = load_lib()
        self._h = None
        vp, ci, cs, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t
        L = self._lib
        L.pfhip_mos_create_from_files.argtypes = [cs, cs, ci, ctypes.POINTER(vp)]
        L.pfhip_mos_create_from_memory.argtypes = [vp, sz, cs, ci, ctypes.POINTER(vp)]
        L.pfhip_mos_destroy.argtypes = [vp]
        L.pfhip_mos_destroy.restype = None
        L.pfhip_mos_set_workspace.argtypes = [vp, sz]
        for fn in (L.pfhip_mos_score, L.pfhip_mos_score_s16):
            fn.argtypes = [vp, vp, vp, ci, ci, ctypes.POINTER(_Result)]
        for fn in (L.pfhip_mos_score_windows, L.pfhip_mos_score_windows_s16):
            fn.argtypes = [vp, vp, vp, ci, vp, vp, vp, sz, ctypes.POINTER(sz)]

    def InitMos(self, primary, p808=None, device=0):
        """primary / p808: paths of sig_bak_ovr.onnx and model_v8.onnx (read by the C++ reader), or primary = (manifest, blob), a
        container of kind "dnsmos".  Without the P.808 net the `p808` field of every result is NaN."""
        self.close()
        h = ctypes.c_void_p()
        if isinstance(primary, tuple):
            import json
            man, blob = primary
            blob = np.ascontiguousarray(blob, np.float32)
            st = self._lib.pfhip_mos_create_from_memory(blob.ctypes.data, blob.nbytes, json.dumps(man).encode(), int(device), ctypes.byref(h))
        else:
            st = self._lib.pfhip_mos_create_from_files(str(primary).encode(), None if p808 is None else str(p808).encode(), int(device),
                                                       ctypes.byref(h))
        _check(self._lib, st)
        self._h = h
        return self

    def set_workspace(self, n_bytes):
        _check(self._lib, self._lib.pfhip_mos_set_workspace(self._need(), int(n_bytes)))

    def close(self):
        if self._h is not None:
            self._lib.pfhip_mos_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _need(self):
        if self._h is None:
            raise PfhipError("InitMos first")
        return self._h

    def _pack(self, clips):
        arrs = [np.ascontiguousarray(c).reshape(-1) for c in clips]
        kinds = {a.dtype for a in arrs}
        if len(kinds) > 1 or (kinds and next(iter(kinds)) not in (np.dtype("float32"), np.dtype("int16"))):
            raise PfhipError("score takes float32 or int16 arrays, all of one kind")
        s16 = bool(arrs) and arrs[0].dtype == np.dtype("int16")
        ptrs = (ctypes.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
        lens = np.array([a.size for a in arrs], np.int64)
        return arrs, s16, ptrs, lens

    def score_windows(self, clips):
        """clips: float32 arrays in [-1, 1] or int16 arrays (all of one kind), 16 kHz.  Returns (num_hops [n_clips], n_scored [n_clips],
        raw [sum n_scored, 4] float32 = (p808, sig, bak, ovr) of every scored window, clip after clip)."""
        h = self._need()
        arrs, s16, ptrs, lens = self._pack(clips)
        cap = sum(windows_of(a.size)[2] for a in arrs)
        hops, scored = np.zeros(max(len(arrs), 1), np.int32), np.zeros(max(len(arrs), 1), np.int32)
        raw, n = np.zeros((max(cap, 1), 4), np.float32), ctypes.c_size_t()
        fn = self._lib.pfhip_mos_score_windows_s16 if s16 else self._lib.pfhip_mos_score_windows
        _check(self._lib, fn(h, ptrs, lens.ctypes.data, len(arrs), hops.ctypes.data, scored.ctypes.data, raw.ctypes.data, cap, ctypes.byref(n)))
        return [int(v) for v in hops[:len(arrs)]], [int(v) for v in scored[:len(arrs)]], raw[:n.value].copy()

    def score(self, clips, personalized=False):
        """One dict per clip: num_hops, n_scored, p808, sig_raw, bak_raw, ovr_raw, sig, bak, ovr."""
        h = self._need()
        arrs, s16, ptrs, lens = self._pack(clips)
        res = (_Result * max(len(arrs), 1))()
        fn = self._lib.pfhip_mos_score_s16 if s16 else self._lib.pfhip_mos_score
        _check(self._lib, fn(h, ptrs, lens.ctypes.data, len(arrs), 1 if personalized else 0, res))
        return [{k: getattr(r, k) for k, _ in _Result._fields_} for r in res[:len(arrs)]]
