"""CPU: the small Paraformer's model directory (d_model 320, four heads of 80, FFN 1280 / 1280) in the reference's file layout
(tests/ref_layout.py) through the C++ reader (pfhip_read_model_files) and the Python converter (convert.py): the same container,
bit for bit, carrying the widths config.yaml states — the reference takes whatever encoder_conf / decoder_conf say
(onnxruntime/src/paraformer.cpp:213-232).  No compute call: runs without a GPU."""
import importlib
import os

import numpy as np
import pytest

import ref_layout as RL


@pytest.fixture(scope="module")
def mods(pkg):
    return pkg, importlib.import_module(pkg.__name__ + ".convert"), importlib.import_module(pkg.__name__ + ".weights")


def test_config_constants(mods):
    _, _, wt = mods
    s = wt.PARAFORMER_SMALL
    assert (s["d_model"], s["n_head"], s["ffn"], s["dec_ffn"]) == (320, 4, 1280, 1280) and s["d_model"] // s["n_head"] == 80
    c = wt.small_config_320()
    assert (c["d_model"], c["n_head"], c["ffn"], c["dec_ffn"], c["enc_layers"], c["dec_layers"], c["vocab"]) == (320, 4, 1280, 1280, 3, 2, 1003)
    assert wt.small_config_320(vocab=97)["vocab"] == 97
    big = wt.small_config()
    assert (big["d_model"], big["n_head"], big["ffn"]) == (512, 4, 2048)          # small_config stays the 512-wide one


@pytest.mark.parametrize("online", [True, False])
def test_320_directory_converts_bit_for_bit_in_both_loaders(mods, tmp_path, monkeypatch, online):
    pkg, conv, wt = mods
    monkeypatch.setenv("PFHIP_MODEL_CACHE", "0")
    cfg = wt.small_config_320(enc_layers=2, dec_layers=2, vocab=97)
    man, blob = wt.synth_weights(cfg, seed=320)
    d = tmp_path / "small"
    RL.write_asr_dir(str(d), conv, man, blob, cfg, online=online)
    second = str(d / "decoder.onnx") if online else None
    man2, blob2, cached = pkg.read_model_files("asr", str(d / "model.onnx"), second=second, cmvn=str(d / "am.mvn"), config=str(d / "config.yaml"))
    assert not cached and man2["tensors"] == man["tensors"] and man2["total_bytes"] == man["total_bytes"]
    assert np.array_equal(blob2, blob)
    c2 = man2["config"]
    assert (c2["d_model"], c2["n_head"], c2["ffn"], c2["dec_ffn"]) == (320, 4, 1280, 1280)
    assert c2["enc_layers"] == 2 and c2["dec_layers"] == 2 and c2["vocab"] == 97 and "dec_n_head" not in c2
    man3, blob3, _ = conv.convert_model_dir("asr", str(d))
    assert man3["tensors"] == man2["tensors"] and np.array_equal(blob3, blob2)
    for k in ("d_model", "n_head", "ffn", "dec_ffn", "enc_layers", "dec_layers", "vocab", "kernel"):
        assert man3["config"][k] == c2[k], k
    assert "dec_n_head" not in man3["config"]


def test_decoder_widths_that_differ_from_the_encoders_are_honoured(mods, tmp_path, monkeypatch):
    """decoder_conf.linear_units and decoder_conf.attention_heads are the decoder's own: FFN 1280 in the encoder and 640 in the
    decoder (the tensors have those shapes), 4 heads in the encoder and 2 stated for the decoder."""
    pkg, conv, wt = mods
    monkeypatch.setenv("PFHIP_MODEL_CACHE", "0")
    cfg = wt.small_config_320(enc_layers=1, dec_layers=1, vocab=53, dec_ffn=640)
    man, blob = wt.synth_weights(cfg, seed=321)
    d = tmp_path / "mixed"
    RL.write_asr_dir(str(d), conv, man, blob, cfg)
    y = open(d / "config.yaml").read()
    head, dec = y.split("decoder_conf:\n")
    assert "attention_heads" not in dec
    with open(d / "config.yaml", "w") as f:
        f.write(head + "decoder_conf:\n    attention_heads: 2\n" + dec)
    man2, blob2, _ = pkg.read_model_files("asr", str(d / "model.onnx"), cmvn=str(d / "am.mvn"), config=str(d / "config.yaml"))
    c2 = man2["config"]
    assert (c2["ffn"], c2["dec_ffn"], c2["n_head"], c2["dec_n_head"]) == (1280, 640, 4, 2)
    assert man2["tensors"]["dec.0.ffn1.w"]["shape"] == [640, 320] and man2["tensors"]["enc.0.ffn1.w"]["shape"] == [1280, 320]
    assert np.array_equal(blob2, blob)
    man3, blob3, _ = conv.convert_model_dir("asr", str(d))
    assert np.array_equal(blob3, blob2) and man3["tensors"] == man2["tensors"]
    assert (man3["config"]["dec_ffn"], man3["config"]["n_head"], man3["config"]["dec_n_head"]) == (640, 4, 2)


def test_header_declares_the_head_width_query(mods):
    pkg, _, _ = mods
    assert "pfhip_head_dim" in pkg.ABI_SYMBOLS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pfhip.h")).read()
    assert "int pfhip_head_dim(const pfhip_model* m);" in text and "paraformer.cpp:225" in text
    assert hasattr(pkg.load_lib(), "pfhip_head_dim") and hasattr(pkg.load_lib(), "pfhip_op_window_attention_hd")
