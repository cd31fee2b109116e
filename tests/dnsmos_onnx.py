"""Test helper: writes an .onnx of each DNSMOS family from the fixture tensors (tests/golden/dnsmos_*.npz), node for node the shape
of the real exports (tensor names, operator order, attributes), with tests/onnx_writer.py's protobuf primitives — so that the
file-reading path can be driven where the reference tree is absent."""
import numpy as np

import dnsmos_ref as R
from onnx_writer import attr_int, key, ld, model, node, s, tensor, value_info, varint


def attr_ints(name, vals):
    return s(1, name) + b"".join(key(8, 0) + varint(int(v)) for v in vals) + key(20, 0) + varint(7)


def attr_str(name, text):
    return s(1, name) + ld(4, text.encode()) + key(20, 0) + varint(3)


def _tail(W, net, nodes, cur, drop=()):
    """Conv / Relu / MaxPool groups, ReduceMax and the three dense layers behind `cur` (an NCHW value)."""
    conv_attrs = [attr_str("auto_pad", "NOTSET"), attr_ints("dilations", [1, 1]), attr_int("group", 1), attr_ints("kernel_shape", [3, 3]),
                  attr_ints("pads", [1, 1, 1, 1]), attr_ints("strides", [1, 1])]
    for i, (name, pool) in enumerate(net["convs"]):
        nodes.append(node("Conv", [cur, f"{name}/kernel:0", f"{name}/bias:0"], [f"conv_out{i}"], name, conv_attrs))
        nodes.append(node("Relu", [f"conv_out{i}"], [f"{net['prefix']}/{name}/Relu:0"], f"Relu{i}"))
        cur = f"{net['prefix']}/{name}/Relu:0"
        if pool:
            nodes.append(node("MaxPool", [cur], [cur + "_pooling0"], cur + "_pooling",
                              [attr_ints("kernel_shape", [2, 2]), attr_ints("strides", [2, 2])]))
            cur += "_pooling0"
    nodes.append(node("Transpose", [cur], ["push_transpose_out_0"], "PushTranspose_0", [attr_ints("perm", [0, 2, 3, 1])]))
    nodes.append(node("ReduceMax", ["push_transpose_out_0"], ["gmax"], "global_max", [attr_ints("axes", [1, 2]), attr_int("keepdims", 0)]))
    cur = "gmax"
    for i, d in enumerate(net["dense"]):
        p = f"{net['prefix']}/{d}"
        nodes.append(node("MatMul", [cur, f"{p}/MatMul/ReadVariableOp/resource:0"], [f"{p}/MatMul:0"], f"{p}/MatMul_add"))
        out = "Identity:0" if i == 2 else f"{p}/BiasAdd:0"
        nodes.append(node("Add", [f"{p}/MatMul:0", f"{p}/BiasAdd/ReadVariableOp/resource:0"], [out], f"{p}/BiasAdd_add"))
        cur = out
        if i < 2:
            nodes.append(node("Relu", [cur], [f"{p}/Relu:0"], f"{p}/Relu"))
            cur = f"{p}/Relu:0"
    inits = [tensor(k, v) for k, v in W.items() if k not in drop]
    return nodes, inits


def primary_onnx(W, drop=(), rename=None):
    """sig_bak_ovr.onnx from the fixture tensors; `drop`: initialisers left out (a damaged file); `rename`: other names for the two
    STFT kernels in the nodes that read them (W then holds them under those names)."""
    r = lambda n: (rename or {}).get(n, n)
    pre = "mos_estimator_logpow"
    perm = [attr_ints("perm", [0, 2, 1])]
    c1 = [attr_str("auto_pad", "VALID"), attr_ints("dilations", [1]), attr_int("group", 1), attr_ints("kernel_shape", [1]), attr_ints("strides", [1])]
    nodes = [
        node("Slice", ["input_1"] + [f"input_1:01_cropping_{x}" for x in ("start", "end", "axes", "steps")], ["crop0"], "input_1:01_cropping"),
        node("Slice", ["input_1"] + [f"input_1:01_cropping_{x}1" for x in ("start", "end", "axes", "steps")], ["crop1"], "input_1:01_cropping_1"),
        node("Reshape", ["crop0", "shape_tensor"], ["resh0"], f"{pre}/Reshape_reshape"),
        node("Reshape", ["crop1", "shape_tensor1"], ["resh1"], f"{pre}/Reshape_1_reshape"),
        node("Concat", ["resh0", "resh1"], ["frames"], f"{pre}/concat_concat", [attr_int("axis", 2)]),
        node("Transpose", ["frames"], ["adj7"], "Transpose15", perm),
        node("Transpose", ["frames"], ["adj8"], "Transpose17", perm),
        node("Conv", ["adj7", r("time2freq/stft-real/kernel:0")], ["cre"], "stft-real", c1),
        node("Conv", ["adj8", r("time2freq/stft-imag/kernel:0")], ["cim"], "stft-imag", c1),
        node("Transpose", ["cre"], ["re"], "Transpose16", perm),
        node("Transpose", ["cim"], ["im"], "Transpose18", perm),
        node("Mul", ["re", "re"], ["re2"], f"{pre}/time2freq/Square"),
        node("Mul", ["im", "im"], ["im2"], f"{pre}/time2freq/Square_1"),
        node("Add", ["re2", "im2"], ["p2"], f"{pre}/time2freq/Add"),
        node("Sqrt", ["p2"], ["mag"], f"{pre}/time2freq/Sqrt"),
        node("Pow", ["mag", f"{pre}/pow/y:0"], ["pw"], f"{pre}/pow"),
        node("Max", [f"{pre}/Maximum/x:0", "pw"], ["fl"], f"{pre}/Maximum_max"),
        node("Log", ["fl"], ["lg"], f"{pre}/Log"),
        node("Div", ["lg", f"{pre}/truediv/y:0"], [f"{pre}/truediv:0"], f"{pre}/truediv"),
        node("Unsqueeze", [f"{pre}/truediv:0"], ["exp"], f"{pre}/ExpandDims", [attr_ints("axes", [3])]),
        node("Transpose", ["exp"], ["adj6"], "Transpose13", [attr_ints("perm", [0, 3, 1, 2])]),
    ]
    nodes, inits = _tail(W, R.PRIMARY, nodes, "adj6", drop)
    return model(nodes, inits, [value_info("input_1", dims=("N", 144160))], [value_info("Identity:0", dims=("N", 3))])


def p808_onnx(W, drop=()):
    nodes = [
        node("Unsqueeze", ["input_1"], ["exp"], "mos_estimator_small_1/ExpandDims", [attr_ints("axes", [3])]),
        node("Transpose", ["exp"], ["adj4"], "Transpose9", [attr_ints("perm", [0, 3, 1, 2])]),
    ]
    nodes, inits = _tail(W, R.P808, nodes, "adj4", drop)
    return model(nodes, inits, [value_info("input_1", dims=("N", 900, 120))], [value_info("Identity:0", dims=("N", 1))])


def not_dnsmos_onnx():
    """A graph of another family (a LayerNormalization and a MatMul, as a Paraformer block starts)."""
    g = np.ones(8, np.float32)
    nodes = [node("LayerNormalization", ["x", "norm.weight", "norm.bias"], ["h"], "/encoder/norm/LayerNormalization"),
             node("MatMul", ["h", "w"], ["y"], "/encoder/linear/MatMul")]
    return model(nodes, [tensor("norm.weight", g), tensor("norm.bias", g), tensor("w", np.eye(8, dtype=np.float32))], [value_info("x")],
                 [value_info("y")])
