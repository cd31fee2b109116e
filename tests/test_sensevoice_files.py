"""CPU: a SenseVoiceSmall model directory in the reference's file layout — a synthetic model.onnx with the upstream state-dict names
(recalled from upstream FunASR), am.mvn, config.yaml — through the C++ reader (pfhip_read_model_files) and the Python converter
(convert.py): the same container, bit for bit; the kinds are told apart by the initialisers (ctc.ctc_lo.* present, no decoder), in
both directions; the conversion cache beside the source is reused on the second read.  No compute call: runs without a GPU."""
import importlib
import os

import numpy as np
import pytest

import ref_layout as RL
import sensevoice_ref as R

CONFIG_KEYS = ("kind", "d_model", "n_head", "ffn", "enc_layers", "tp_layers", "dec_layers", "dec_ffn", "kernel", "vocab", "blank_id", "n_mels",
               "lfr_m", "lfr_n", "fs")


@pytest.fixture(scope="module")
def mods(pkg):
    return pkg, importlib.import_module(pkg.__name__ + ".convert"), importlib.import_module(pkg.__name__ + ".weights")


@pytest.fixture(scope="module")
def svs(mods):
    _, _, wt = mods
    cfg = wt.small_config_svs(enc_layers=2, tp_layers=3, vocab=97)
    return wt.synth_svs_weights(cfg, seed=41)


def paths(d):
    return dict(cmvn=str(d / "am.mvn"), config=str(d / "config.yaml"))


@pytest.mark.parametrize("wrapped", [False, True])
def test_directory_converts_bit_for_bit_in_both_loaders(mods, svs, tmp_path, monkeypatch, wrapped):
    """wrapped: modules named encoder.model.encoders0... as FunASR's export wrappers may leave them."""
    pkg, conv, wt = mods
    monkeypatch.setenv("PFHIP_MODEL_CACHE", "0")
    man, blob = svs
    d = tmp_path / "SenseVoiceSmall"
    R.write_model_dir(str(d), conv, man, blob, wrapper_model_component=wrapped)
    for kind in ("sensevoice", "asr"):                    # "asr" recognises the kind from the initialisers
        man2, blob2, cached = pkg.read_model_files(kind, str(d / "model.onnx"), **paths(d))
        assert not cached and man2["tensors"] == man["tensors"] and man2["total_bytes"] == man["total_bytes"]
        assert np.array_equal(blob2, blob)
        c2 = man2["config"]
        assert c2["kind"] == "sensevoice" and (c2["enc_layers"], c2["tp_layers"], c2["dec_layers"], c2["vocab"], c2["blank_id"]) == (2, 3, 0, 97, 0)
    man3, blob3, files = conv.convert_model_dir("sensevoice", str(d))
    assert man3["tensors"] == man2["tensors"] and man3["total_bytes"] == man2["total_bytes"] and np.array_equal(blob3, blob2)
    for k in CONFIG_KEYS:
        assert man3["config"][k] == c2[k], k
    assert [os.path.basename(f) for f in files] == ["model.onnx", "am.mvn", "config.yaml"]
    man4, blob4, _ = conv.convert_model_dir("asr", str(d))
    assert man4["config"]["kind"] == "sensevoice" and np.array_equal(blob4, blob3)


def test_a_paraformer_directory_is_not_taken_for_sensevoice_and_vice_versa(mods, svs, tmp_path, monkeypatch):
    pkg, conv, wt = mods
    monkeypatch.setenv("PFHIP_MODEL_CACHE", "0")
    pcfg = wt.small_config(enc_layers=1, dec_layers=1, vocab=53)
    pman, pblob = wt.synth_weights(pcfg, seed=42)
    pd = tmp_path / "paraformer"
    RL.write_asr_dir(str(pd), conv, pman, pblob, pcfg)
    with pytest.raises(pkg.PfhipError) as e:
        pkg.read_model_files("sensevoice", str(pd / "model.onnx"), **paths(pd))
    assert e.value.status == 3 and "not a SenseVoice model" in str(e.value)               # PFHIP_ERR_FORMAT
    with pytest.raises(ValueError):
        conv.convert_model_dir("sensevoice", str(pd))
    man2, blob2, _ = pkg.read_model_files("asr", str(pd / "model.onnx"), **paths(pd))
    assert "kind" not in man2["config"] and "dec.out.w" in man2["tensors"] and np.array_equal(blob2, pblob)
    # a SenseVoice directory read as "asr" is not forced into a Paraformer: no pred.* / dec.* tensor is asked of it
    man, blob = svs
    sd = tmp_path / "SenseVoiceSmall"
    R.write_model_dir(str(sd), conv, man, blob)
    man3, _, _ = pkg.read_model_files("asr", str(sd / "model.onnx"), **paths(sd))
    assert man3["config"]["kind"] == "sensevoice" and not any(k.startswith(("pred.", "dec.")) for k in man3["tensors"])
    # a CTC head beside a decoder (a Paraformer trained with a CTC loss) stays a Paraformer
    state = RL.upstream_state(conv.paraformer_name_map(pcfg), pman, pblob, RL.asr_expand)
    state["ctc.ctc_lo.weight"] = np.zeros((53, 512), np.float32)
    state["ctc.ctc_lo.bias"] = np.zeros(53, np.float32)
    assert not conv.is_sensevoice(state)
    RL.write_onnx(str(pd / "model.onnx"), state)
    man5, blob5, _ = pkg.read_model_files("asr", str(pd / "model.onnx"), **paths(pd))
    assert "kind" not in man5["config"] and np.array_equal(blob5, pblob)


def test_cache_is_reused_on_the_second_read(mods, svs, tmp_path, monkeypatch):
    pkg, conv, _ = mods
    monkeypatch.delenv("PFHIP_MODEL_CACHE", raising=False)
    man, blob = svs
    d = tmp_path / "SenseVoiceSmall"
    R.write_model_dir(str(d), conv, man, blob)
    _, blob1, cached1 = pkg.read_model_files("sensevoice", str(d / "model.onnx"), **paths(d))
    assert not cached1 and os.path.exists(d / "model.pfhip.bin") and os.path.exists(d / "model.pfhip.json")
    man2, blob2, cached2 = pkg.read_model_files("sensevoice", str(d / "model.onnx"), **paths(d))
    assert cached2 and np.array_equal(blob2, blob1) and man2["config"]["kind"] == "sensevoice"
    # a source that changes invalidates it
    with open(d / "config.yaml", "a") as f:
        f.write("# touched\n")
    _, _, cached3 = pkg.read_model_files("sensevoice", str(d / "model.onnx"), **paths(d))
    assert not cached3


def test_missing_tensor_fails_loudly(mods, svs, tmp_path, monkeypatch):
    pkg, conv, _ = mods
    monkeypatch.setenv("PFHIP_MODEL_CACHE", "0")
    man, blob = svs
    d = tmp_path / "SenseVoiceSmall"
    state = R.write_model_dir(str(d), conv, man, blob)
    del state["encoder.tp_norm.weight"]
    RL.write_onnx(str(d / "model.onnx"), state)
    with pytest.raises(pkg.PfhipError) as e:
        pkg.read_model_files("sensevoice", str(d / "model.onnx"), **paths(d))
    assert "tp.norm.g" in str(e.value)
