"""CPU: the numpy restatement of SenseVoiceSmall (tests/sensevoice_ref.py) — hand-derived known answers for the CTC collapse and the
text assembly of CTCSearch (onnxruntime/src/sensevoice-small.cpp:323-377), the order and positions of the prompt rows, lid_map, and one
encoder layer + one tp layer against torch.nn modules assembled as in test_oracle_vs_torch_nn.py, loaded through the upstream
state_dict names of convert.sensevoice_name_map."""
import importlib

import numpy as np
import pytest

import sensevoice_ref as R
from oracle import frontend as FE
from oracle import paraformer as P

A, B, C = 7, 8, 9


def test_collapse_known_answers():
    assert R.ctc_collapse([A, A, 0, A, B, B, 0, 0, C]) == ([A, A, B, C], [0, 3, 4, 8])       # a a _ a b b _ _ c -> a a b c
    assert R.ctc_collapse([0, 0, 0, 0]) == ([], [])                                             # all blank
    assert R.ctc_collapse([0, 0, A, A, 0]) == ([A], [2])                                        # leading blanks
    assert R.ctc_collapse([A, 0, A]) == ([A, A], [0, 2])                                        # a blank separates equal ids
    assert R.ctc_collapse([]) == ([], [])
    assert R.ctc_collapse([3, 3, 5, 3], blank=5) == ([3, 3], [0, 3])                            # the blank id is the model's


VOCAB = ["<blank>", "<|zh|>", "<|en|>", "<|NEUTRAL|>", "<|Speech|>", "<|withitn|>", "<|woitn|>", "▁hello", "▁world", "你", "好", "."]


def test_text_and_the_three_trailing_space_cases():
    tags_en_itn, tags_zh_itn, tags_zh_wo = [2, 3, 4, 5], [1, 3, 4, 5], [1, 3, 4, 6]
    assert R.ctc_text(tags_en_itn + [7, 8, 11], VOCAB) == " hello world. "      # with ITN, English: one space is added
    assert R.ctc_text(tags_zh_itn + [9, 10, 11], VOCAB) == "你好."       # with ITN, another language: nothing is added
    assert R.ctc_text(tags_zh_wo + [9, 10], VOCAB) == "你好 "            # without ITN: a space is added
    assert R.ctc_text(tags_en_itn, VOCAB) == " "                                  # tags only: no text, English with ITN
    # fewer than four kept ids: no tags are read (the reference reads tokens[3] after checking size() >= 3), no text, the no-ITN space
    assert R.ctc_text([2, 3, 4], VOCAB) == " " and R.ctc_text([], VOCAB) == " "


def test_lid_map_and_textnorm():
    assert [R.lid_of(s) for s in ("auto", "zh", "en", "yue", "ja", "ko", "nospeech")] == [0, 3, 4, 7, 11, 12, 13]
    assert R.lid_of("fr") == 0 and R.lid_of("") == 0
    assert R.textnorm_of(True) == 14 and R.textnorm_of(False) == 15


def test_prompt_row_order_and_positions():
    rng = np.random.default_rng(1)
    E = rng.standard_normal((16, 560)).astype(np.float32)
    feats = rng.standard_normal((5, 560)).astype(np.float32)
    x = R.encoder_input(feats, E, 7, 14)
    assert x.shape == (9, 560)
    assert np.array_equal(x[0], E[7]) and np.array_equal(x[1], E[1]) and np.array_equal(x[2], E[2]) and np.array_equal(x[3], E[14])
    assert np.array_equal(x[4:], feats)
    # scaled by sqrt(512), then the position encoding of positions 1 .. T + 4 at depth 560: the prompt rows take positions 1 .. 4
    emb = P.embed(x, 512)
    pe = FE.pos_emb(9, 560)
    assert np.allclose(emb, x * np.float32(np.sqrt(512.0)) + pe, atol=1e-6)
    assert np.allclose(emb[3] - x[3] * np.float32(np.sqrt(512.0)), FE.pos_emb(4, 560)[3], atol=1e-5)


def test_head64_is_a_log_softmax_with_first_maximum():
    rng = np.random.default_rng(2)
    enc = rng.standard_normal((6, 32)).astype(np.float32)
    w = rng.standard_normal((10, 32)).astype(np.float32)
    w[4] = w[2]
    b = np.zeros(10, np.float32)
    b[[2, 4]] = 50.0
    lp = R.ctc_head64(enc, w, b)
    assert np.allclose(np.exp(lp).sum(axis=1), 1.0) and (lp.argmax(axis=1) == 2).all()


def test_encoder_and_tp_layer_against_torch_nn(pkg):
    """enc.0 (560 -> 512, no residual) and tp.0 (512 -> 512, residual) as torch modules loaded through the upstream names."""
    torch = pytest.importorskip("torch")
    TV = importlib.import_module("test_oracle_vs_torch_nn")
    conv, wt = importlib.import_module(pkg.__name__ + ".convert"), importlib.import_module(pkg.__name__ + ".weights")
    cfg = wt.small_config_svs(enc_layers=1, tp_layers=1, vocab=53)
    man, blob = wt.synth_svs_weights(cfg, seed=5)
    W = P.Weights(man, blob)
    names = conv.sensevoice_name_map(cfg)
    assert set(names) == set(man["tensors"]) - {"cmvn.mean", "cmvn.istd"}
    state = {}
    for k, key in names.items():
        a = W[k]
        state[key] = TV.t(a[:, None, :] if k.endswith("fsmn.w") else a)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((13, 560)).astype(np.float32)
    enc0 = TV.load(TV.EncLayer(560, 512, 4, 2048, 11), state, "encoder.encoders0.0")
    tp0 = TV.load(TV.EncLayer(512, 512, 4, 2048, 11), state, "encoder.tp_encoders.0")
    after, tpn = torch.nn.LayerNorm(512, eps=1e-12), torch.nn.LayerNorm(512, eps=1e-12)
    TV.load(after, state, "encoder.after_norm"); TV.load(tpn, state, "encoder.tp_norm")
    with torch.no_grad():
        y0 = enc0(TV.t(x)[None])
        y1 = tpn(tp0(after(y0)))[0]
    n0 = P.encoder_layer(x, W, "enc.0.", 4)
    TV.close(y0[0], n0)
    n1 = P.encoder_layer(P.layer_norm(n0, W["enc.after_norm.g"], W["enc.after_norm.b"]), W, "tp.0.", 4)      # width 512: with its residual
    TV.close(y1, P.layer_norm(n1, W["tp.norm.g"], W["tp.norm.b"]))
    want = R.encoder(x, W)                       # embed() is part of encoder(): undo it for the module chain's input
    emb = P.embed(x, 512)
    with torch.no_grad():
        y = tpn(tp0(after(enc0(TV.t(emb)[None]))))[0]
    TV.close(y, want)
    ctc = torch.nn.Linear(512, 53)
    TV.load(ctc, state, "ctc.ctc_lo")
    with torch.no_grad():
        lp = torch.log_softmax(ctc(y).double(), dim=-1).numpy()
    assert np.abs(lp - R.ctc_head64(want, W["ctc.w"], W["ctc.b"])).max() < 1e-3
