"""The large CT-Transformer's shape (d_model 516, twelve heads of 43, ffn 2048; two blocks and 300 tokens here) through the loaders:
a directory in the reference's layout (tests/ref_layout.py) read by the C++ reader (csrc/model_files.cpp load_punc) and by its
Python twin (convert.py).  Both take d_model from embed.weight and ffn from the first feed-forward weight; encoder_conf may leave
output_size / linear_units out and may not contradict the tensors.  CPU tests need no device; the two GPU tests run that
directory through the Python and the C++ adapters against the oracle on the original tensors.  The shape is recalled from the
upstream config, not read from a real file: UPSTREAM names stay unverified."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import ref_layout as RL
from oracle import ct_transformer as C
from oracle import paraformer as P

CJK = [chr(0x4E00 + i) for i in range(200)]
ENG = [f"w{i}" for i in range(95)] + ["hello", "world", "i'm", "a.i."]
TOKENS = ["<unk>"] + CJK + ENG                       # 300
TIE_GAP = 2e-3


@pytest.fixture(scope="module")
def mods(pkg):
    return pkg, importlib.import_module(pkg.__name__ + ".convert"), importlib.import_module(pkg.__name__ + ".weights")


@pytest.fixture(scope="module")
def large_dir(mods, tmp_path_factory):
    pkg, conv, wt = mods
    cfg = dict(wt.CT_TRANSFORMER, vocab=len(TOKENS), d_model=516, n_head=12, ffn=2048, layers=2)
    man, blob = wt.synth_punc_weights(cfg, seed=516)
    d = tmp_path_factory.mktemp("punc_large")
    RL.write_punc_dir(str(d), conv, man, blob, TOKENS)
    return d, man, blob


def read(pkg, d, config="config.yaml"):
    return pkg.read_model_files("punc", str(d / "model.onnx"), config=str(d / config))


def test_directory_comes_back_bit_for_bit_from_both_readers(mods, large_dir, monkeypatch):
    pkg, conv, wt = mods
    monkeypatch.setenv("PFHIP_MODEL_CACHE", "0")
    d, man, blob = large_dir
    man2, blob2, cached = read(pkg, d)
    assert not cached and man2["tensors"] == man["tensors"] and man2["total_bytes"] == man["total_bytes"]
    assert np.array_equal(blob2, blob)
    for k, v in (("vocab", 300), ("d_model", 516), ("n_head", 12), ("ffn", 2048), ("layers", 2), ("kernel", 11), ("n_punc", 6)):
        assert man2["config"][k] == v, k
    man3, blob3, _ = conv.convert_model_dir("punc", str(d))
    assert man3["tensors"] == man2["tensors"] and np.array_equal(blob3, blob2)
    for k in ("vocab", "d_model", "n_head", "ffn", "layers", "kernel", "n_punc"):
        assert man3["config"][k] == man2["config"][k], k


def rewrite_config(d, name, edit):
    lines = open(d / "config.yaml", encoding="utf-8").read().splitlines(keepends=True)
    with open(d / name, "w", encoding="utf-8") as f:
        f.writelines(edit(lines))


def test_widths_come_from_the_tensors_when_the_config_leaves_them_out(mods, large_dir, monkeypatch, tmp_path):
    pkg, conv, wt = mods
    monkeypatch.setenv("PFHIP_MODEL_CACHE", "0")
    d, man, blob = large_dir
    rewrite_config(d, "no_sizes.yaml", lambda ls: [l for l in ls if "output_size" not in l and "linear_units" not in l])
    assert "output_size" not in open(d / "no_sizes.yaml", encoding="utf-8").read()
    man2, blob2, _ = read(pkg, d, "no_sizes.yaml")
    assert man2["tensors"] == man["tensors"] and np.array_equal(blob2, blob)
    assert man2["config"]["d_model"] == 516 and man2["config"]["ffn"] == 2048
    # the Python twin reads <dir>/config.yaml: a copy of the directory with the shortened file under that name
    t = tmp_path / "twin"
    os.makedirs(t)
    os.symlink(d / "model.onnx", t / "model.onnx")
    with open(t / "config.yaml", "w", encoding="utf-8") as f:
        f.write(open(d / "no_sizes.yaml", encoding="utf-8").read())
    man3, blob3, _ = conv.convert_model_dir("punc", str(t))
    assert man3["tensors"] == man["tensors"] and np.array_equal(blob3, blob)
    assert man3["config"]["d_model"] == 516 and man3["config"]["ffn"] == 2048


@pytest.mark.parametrize("key,stated,has", [("output_size", 512, 516), ("linear_units", 1024, 2048)])
def test_a_config_that_contradicts_the_tensors_is_refused(mods, large_dir, monkeypatch, tmp_path, key, stated, has):
    pkg, conv, wt = mods
    monkeypatch.setenv("PFHIP_MODEL_CACHE", "0")
    d, man, blob = large_dir
    name = f"wrong_{key}.yaml"
    rewrite_config(d, name, lambda ls: [l.replace(f"{key}: {has}", f"{key}: {stated}") for l in ls])
    assert f"{key}: {stated}" in open(d / name, encoding="utf-8").read()
    with pytest.raises(pkg.PfhipError, match=rf"{key} is {stated} but .* has {has}"):
        read(pkg, d, name)
    t = tmp_path / "twin"
    os.makedirs(t)
    os.symlink(d / "model.onnx", t / "model.onnx")
    with open(t / "config.yaml", "w", encoding="utf-8") as f:
        f.write(open(d / name, encoding="utf-8").read())
    with pytest.raises(ValueError, match=rf"{key} is {stated} but .* has {has}"):
        conv.convert_model_dir("punc", str(t))


# ---- GPU: the directory through the adapters ------------------------------------------------------------------------------------

def oracle_with_gap(W):
    """The oracle's Infer plus the smallest top-2 gap it has met: the ids and the text below are compared exactly, which means
    something only while no row of the oracle is a near tie (gap >= 2e-3, twice the logits' tolerance)."""
    seen = {"gap": np.inf}

    def infer(ids):
        lg, p = C.infer(np.asarray(ids, np.int32), W)
        top = np.sort(lg[:, :W.cfg["n_punc"] - 1], axis=-1)
        seen["gap"] = min(seen["gap"], float((top[:, -1] - top[:, -2]).min()))
        return p

    return infer, seen


@pytest.mark.gpu
def test_directory_through_the_python_adapter(mods, large_dir, monkeypatch):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    pkg, conv, wt = mods
    monkeypatch.setenv("PFHIP_MODEL_CACHE", "0")
    d, man, blob = large_dir
    W = P.Weights(man, blob)
    infer, seen = oracle_with_gap(W)
    h = pkg.CTTransformerHip().InitPunc(str(d / "model.onnx"), str(d / "config.yaml"))
    for n in (1, 33, 64):
        ids = np.random.default_rng(n).integers(0, len(TOKENS), n).astype(np.int32)
        want = infer(ids)
        assert seen["gap"] >= TIE_GAP, seen
        assert np.array_equal(h.Infer(ids), want), n
    h.close()


def random_text(rng, n_words):
    out = []
    for _ in range(n_words):
        r = rng.random()
        if r < 0.55:
            out.append(CJK[rng.integers(len(CJK))])
        elif r < 0.9:
            w = ENG[rng.integers(len(ENG))]
            out.append((" " if out and out[-1][-1].isascii() else "") + w)
        else:
            out.append("龘")                                     # not in the vocabulary -> <unk>
    return "".join(out).strip()


@pytest.mark.gpu
def test_directory_through_the_cpp_adapter(mods, large_dir, monkeypatch):
    """As tests/test_gpu_punc_text.py drives the `punc_infer` harness: the container the C++ reader makes of the directory, saved
    beside tokens.json, and AddPunc's text against oracle.ct_transformer.add_punc_text on the original tensors."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    pkg, conv, wt = mods
    monkeypatch.setenv("PFHIP_MODEL_CACHE", "0")
    d, man, blob = large_dir
    man2, blob2, _ = read(pkg, d)
    man2["config"]["punc_list"] = list(C.DEFAULT_PUNC_LIST)
    wt.save(str(d / "punc.pfhip"), man2, blob2)
    with open(d / "tokens.json", "w") as f:
        json.dump(TOKENS, f)                                     # ASCII-only file: \\uXXXX escapes
    exe = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "punc_infer")
    rng = np.random.default_rng(516)
    lines = [random_text(rng, n) for n in (1, 5, 20, 21, 47, 130)] + ["hello world"]
    out = subprocess.run([exe, str(d), "offline"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(lines)
    W = P.Weights(man, blob)
    infer, seen = oracle_with_gap(W)
    t2i = {t: i for i, t in enumerate(TOKENS)}
    for g, line in zip(got, lines):
        want = C.add_punc_text(line, infer, t2i)
        assert seen["gap"] >= TIE_GAP, seen
        assert g == "out " + want, (line, g, want)
