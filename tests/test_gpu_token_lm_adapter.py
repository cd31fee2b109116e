"""GPU: a token n-gram language model through the C++ adapter and the handle-API mirror — FunOfflineInit -> FunOfflineLoadTokenLm
(ParaformerHip::InitTokenLm: an ARPA file this test writes, words matched to the model's tokens.json) -> FunASRCtcDecoderInit ->
FunOfflineInferBuffer(dec_handle) with NO hotwords loaded — run through the `offline_infer` harness as
tests/test_gpu_paraformer_bias_adapter.py runs it.

A plain Paraformer from a reference-layout directory with a vocabulary of single CJK characters.  The expected ids of every VAD
segment are hypothesis 0 of the C-ABI call (ParaformerHip.set_token_lm + forward_bias with a graph-less set, the same library) on
that segment's samples, with the model read from the same file; the text is those ids' characters.  The ARPA file likes the
runner-up candidate behind every greedy token, so the search's text differs from the greedy text."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import ref_layout as RL
from test_gpu_cif_stamps_adapter import field, segments
from test_gpu_pipeline import make_file, shape_vad_weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V = 300
BEAMS = (8, 16)                                  # glob_beam, lat_beam: width min(8, 8), beam min(16, 16)
SCALE, BONUS = 0.5, 0.25


def run(args, env=None):
    out = subprocess.run(args, capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert out.returncode == 0, out.stderr + out.stdout[-3000:]
    return out.stdout.splitlines()


def tagged(lines, tag):
    return segments([l[len(tag) + 1:] for l in lines if l.startswith(tag + "_seg ")])


def arpa_for(asr, pcm, segs, tokens):
    """Flat unigrams, and a well-liked bigram (greedy token, the next row's runner-up) for every row of every segment; one word the
    model does not have, which the reader must skip."""
    pairs = set()
    for s, e, ids in segs:
        if len(ids) < 2:
            continue
        cid = asr.forward_ids([pcm[s:e]], nbest=2)["nbest_ids"][0]
        for t in range(len(ids) - 1):
            pairs.add((int(cid[t, 0]), int(cid[t + 1, 1])))
    pairs = sorted(pairs)
    lines = ["", "\\data\\", "ngram 1=%d" % (V + 3), "ngram 2=%d" % len(pairs), "", "\\1-grams:"]
    lines += ["-2.0\t%s\t-0.5" % t for t in tokens] + ["-99\t<s>\t-0.5", "-2.0\t</s>", "-3.0\tnot-a-token\t-0.1", "", "\\2-grams:"]
    lines += ["-0.05\t%s %s" % (tokens[a], tokens[b]) for a, b in pairs] + ["", "\\end\\", ""]
    return "\n".join(lines)


@pytest.fixture(scope="module")
def offline(pkg, weights_mod, tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    tmp = tmp_path_factory.mktemp("pflm")
    conv = importlib.import_module(pkg.__name__ + ".convert")
    pcm = make_file(np.random.default_rng(13))
    s16 = np.clip(np.round(pcm * 32768.0), -32768, 32767).astype("<i2")
    f32 = (s16.astype(np.float32) / 32768.0).astype(np.float32)
    vman, vblob = shape_vad_weights(*weights_mod.synth_vad_weights())
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=V)
    aman, ablob = weights_mod.synth_weights(cfg, seed=43)
    tokens = [chr(0x4E00 + i) for i in range(V)]
    d = tmp / "asr"
    RL.write_asr_dir(str(d), conv, aman, ablob, cfg, vocab_tokens=tokens)
    RL.write_vad_dir(str(tmp / "vad"), conv, vman, vblob)
    s16.tofile(tmp / "long.pcm")
    asr = pkg.ParaformerHip().InitAsr(str(d / "model.onnx"), str(d / "am.mvn"), str(d / "config.yaml"), str(d / "tokens.json"))
    exe = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "offline_infer")
    base = [exe, str(d), str(tmp / "vad"), str(tmp / "long.pcm"), "1", "1", "1", "-", "16000"]
    segs = segments(run(base))
    arpa = tmp / "tokens.arpa"
    arpa.write_text(arpa_for(asr, f32, segs, tokens), encoding="utf-8")
    env = dict(PFHIP_TOKEN_LM=str(arpa), PFHIP_TOKEN_LM_SCALE=str(SCALE), PFHIP_TOKEN_LM_BONUS=str(BONUS))
    beams = ["0", "0", str(BEAMS[0]), str(BEAMS[1])]                 # a decoder handle, no hotword
    yield dict(pkg=pkg, asr=asr, f32=f32, tokens=tokens, segs=segs, arpa=str(arpa), with_lm=run(base + beams, env), without=run(base + beams))
    asr.close()


def test_init_token_lm_then_forward_with_a_decoder_handle_and_no_hotwords(offline):
    o, L = offline, offline["with_lm"]
    pkg, asr, tokens = o["pkg"], o["asr"], o["tokens"]
    assert field(L, "lm_loaded") == "1" and field(L, "dec_handle") == "1" and field(L, "hw_loaded") == "0"
    assert segments(L) == o["segs"]                                  # the passes without a decoder handle never read the model
    lm = pkg.LmGraph.from_arpa(o["arpa"], tokens, scale=SCALE, token_bonus=BONUS, oov_log10=-10.0)
    assert lm.n_skipped == 1
    asr.set_token_lm(lm)
    try:
        got = tagged(L, "dec")
        assert [(s, e) for s, e, _ in got] == [(s, e) for s, e, _ in o["segs"]]
        changed = 0
        for (s, e, ids), (_, _, plain) in zip(got, o["segs"]):
            r = asr.forward_bias([o["f32"][s:e]], [(min(BEAMS[0], 8), min(BEAMS[1], 16), 1, None)])
            want = r["hyps"][0][0][0].tolist() if r["hyps"][0] else []
            assert ids == want and len(ids) == len(plain), (s, e)
            changed += int(ids != plain)
        assert changed >= 1                                          # the model's liking for the runner-ups shows
        assert field(L, "dec_text") == "".join(tokens[i] for _, _, ids in got for i in ids) != field(L, "text")
        assert tagged(L, "hw") == got and field(L, "hw_text") == field(L, "dec_text")      # an empty hotword list changes nothing
    finally:
        asr.set_token_lm(None)


def test_without_a_token_lm_nothing_changes(offline):
    """The same command without the environment variable: a decoder handle without hotwords gives the greedy segments and text."""
    L = offline["without"]
    assert not [l for l in L if l.startswith("lm_loaded")]
    assert tagged(L, "dec") == offline["segs"] and field(L, "dec_text") == field(L, "text")
