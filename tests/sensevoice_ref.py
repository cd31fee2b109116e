"""TEST INFRASTRUCTURE: numpy restatement of what SenseVoiceSmall computes, composed from the oracle's pieces.

The model's widths and wiring are RECALLED from upstream FunASR (no SenseVoice file was available): four prompt rows
E[lid], E[1], E[2], E[textnorm] in front of the LFR / CMVN features (sensevoice-small.cpp:597-640), the whole sequence scaled by
sqrt(d_model) with the sinusoidal position encoding from position 1, SAN-M layers enc.0 .. (the first from 560 to 512 without a
residual), enc.after_norm, the tp layers (all 512 wide, all with a residual), tp.norm, and a CTC head over every row whose
log-softmax is the graph's output.  The head is computed in float64.  CTCSearch (:323-377) is restated as ctc_collapse / ctc_text."""
import numpy as np

from oracle import frontend
from oracle import paraformer as P

F32 = np.float32
LID_MAP = {"auto": 0, "zh": 3, "en": 4, "yue": 7, "ja": 11, "ko": 12, "nospeech": 13}      # sensevoice-small.h:121-129
WORD_START = "▁"


def lid_of(svs_lang):
    """sensevoice-small.cpp:597-602: an unknown string keeps 0."""
    return LID_MAP.get(svs_lang, 0)


def textnorm_of(svs_itn):
    """:603-605: 14 with inverse text normalisation, 15 without."""
    return 14 if svs_itn else 15


def prompt_rows(E, lid, textnorm):
    """The four rows in front of the features, in the graph's order."""
    return np.stack([E[lid], E[1], E[2], E[textnorm]]).astype(F32)


def encoder_input(feats, E, lid, textnorm):
    return np.concatenate([prompt_rows(E, lid, textnorm), feats.astype(F32)], axis=0)


def encoder(x_in, W):
    """[T + 4, 560] -> the rows after tp.norm [T + 4, d]."""
    cfg = W.cfg
    x = P.embed(x_in, cfg["d_model"])
    for i in range(cfg["enc_layers"]):
        x = P.encoder_layer(x, W, f"enc.{i}.", cfg["n_head"])
    x = P.layer_norm(x, W["enc.after_norm.g"], W["enc.after_norm.b"])
    for i in range(cfg["tp_layers"]):
        x = P.encoder_layer(x, W, f"tp.{i}.", cfg["n_head"])
    return P.layer_norm(x, W["tp.norm.g"], W["tp.norm.b"])


def ctc_head64(enc, w, b):
    """float64 log-softmax rows of enc w^T + b."""
    logits = enc.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
    m = logits.max(axis=1, keepdims=True)
    return logits - (m + np.log(np.exp(logits - m).sum(axis=1, keepdims=True)))


def ctc_collapse(frame_ids, blank=0):
    """CTCSearch's loop (:331-343): (kept ids, the frame of each)."""
    ids, frames, prev = [], [], -1
    for t, y in enumerate(int(v) for v in frame_ids):
        if y != blank and y != prev:
            ids.append(y)
            frames.append(t)
        prev = y
    return ids, frames


def ctc_text(tokens, vocab):
    """:344-375 with `vocab` a list of strings.  The first four kept ids are the language / emotion / event / ITN tags; the reference
    reads tokens[3] after checking only size() >= 3 — four are required here, fewer leave the tags empty."""
    lang = itn = ""
    if len(tokens) >= 4:
        lang, itn = vocab[tokens[0]], vocab[tokens[3]]
    text = ""
    for t in tokens[4:]:
        word = vocab[t]
        text += " " + word[len(WORD_START):] if WORD_START in word else word      # the reference's substr(3): the marker's three bytes
    if itn == "<|withitn|>":
        if lang == "<|en|>":
            text += " "
    else:
        text += " "
    return text


def forward_pcm(pcm, W, lid=0, textnorm=15):
    """One utterance: dict(rows, enc [rows, d], logp [rows, V] float64, frame_ids, frame_logp, ids, tok_frame).  Fewer than 400
    samples: no rows at all (the reference returns "" before it runs the graph, :584-587)."""
    cfg = W.cfg
    feats = frontend.extract_feats(pcm, W["cmvn.mean"], W["cmvn.istd"])
    if feats.shape[0] == 0:
        z = np.zeros(0, np.int64)
        return dict(rows=0, enc=np.zeros((0, cfg["d_model"]), F32), logp=np.zeros((0, cfg["vocab"])), frame_ids=z,
                    frame_logp=np.zeros(0), ids=[], tok_frame=[], feats=feats)
    x_in = encoder_input(feats, W["svs.embed.w"], lid, textnorm)
    enc = encoder(x_in, W)
    logp = ctc_head64(enc, W["ctc.w"], W["ctc.b"])
    fid = logp.argmax(axis=1)                              # first maximum wins, as std::max_element
    ids, frames = ctc_collapse(fid, cfg.get("blank_id", 0))
    return dict(rows=x_in.shape[0], enc=enc, logp=logp, frame_ids=fid, frame_logp=logp[np.arange(len(fid)), fid], ids=ids,
                tok_frame=frames, feats=x_in)


def config_yaml(cfg):
    """config.yaml of a SenseVoiceSmall directory as recalled from upstream (encoder_conf.tp_blocks = the layers behind the encoder)."""
    return (f"# written by tests/sensevoice_ref.py\nencoder: SenseVoiceEncoderSmall\nencoder_conf:\n    output_size: {cfg['d_model']}\n"
            f"    attention_heads: {cfg['n_head']}\n    linear_units: {cfg['ffn']}\n    num_blocks: {cfg['enc_layers']}\n"
            f"    tp_blocks: {cfg['tp_layers']}\n    kernel_size: {cfg['kernel']}\n    sanm_shfit: 0\nmodel: SenseVoiceSmall\n"
            "frontend: WavFrontend\nfrontend_conf:\n    fs: 16000\n    window: hamming\n    n_mels: 80\n    frame_length: 25\n    frame_shift: 10\n"
            "    lfr_m: 7\n    lfr_n: 6\ntokenizer: SentencepiecesTokenizer\n")


def write_model_dir(dst, conv, man, blob, vocab_tokens=None, **onnx_kw):
    """A SenseVoiceSmall directory in the reference's file layout (sensevoice-small.cpp:22-56 reads model.onnx, am.mvn, config.yaml,
    tokens.json) from a synthetic container, with the upstream names of convert.sensevoice_name_map in the form the exporter leaves
    (tests/ref_layout.py write_onnx: anonymous transposed MatMul initialisers, named LayerNorm / Conv / embedding parameters)."""
    import json
    import os
    import ref_layout as RL
    cfg = man["config"]
    os.makedirs(dst, exist_ok=True)
    state = RL.upstream_state(conv.sensevoice_name_map(cfg), man, blob, lambda n, a: a[:, None, :] if n.endswith("fsmn.w") else a)
    RL.write_onnx(os.path.join(dst, "model.onnx"), state, **onnx_kw)
    RL.write_mvn(os.path.join(dst, "am.mvn"), RL.view(man, blob, "cmvn.mean"), RL.view(man, blob, "cmvn.istd"))
    with open(os.path.join(dst, "config.yaml"), "w") as f:
        f.write(config_yaml(cfg))
    with open(os.path.join(dst, "tokens.json"), "w", encoding="utf-8") as f:
        json.dump(vocab_tokens if vocab_tokens is not None else [f"<{i}>" for i in range(cfg["vocab"])], f, ensure_ascii=False)
    return state
