"""GPU: hotwords for any Paraformer through the C++ adapter and the handle-API mirror — FunOfflineInit -> FunASRCtcDecoderInit (non-null
for a Paraformer stream) -> FunCtcDecoderLoadHwsRes -> FunOfflineInferBuffer(dec_handle), and one 2-pass case through
FunTpassInferBuffer — run through the `offline_infer` / `tpass_infer` harnesses as tests/test_gpu_cif_stamps_adapter.py runs them.

A plain model from a reference-layout directory with a vocabulary of single CJK characters, so a hotword TEXT of two characters is
two token ids by the decoder's greedy longest match and a token weighs the hotword's score (score x 1 code point).  The expected ids
are hypothesis 0 of the C-ABI call (ParaformerHip.forward_bias, the same library) on each VAD segment's samples with the graph built
here from those ids and weights; batch = 1, so every segment is a forward of its own in the harness as it is here."""
import importlib
import json
import math
import os

import numpy as np
import pytest

import ref_layout as RL
from test_gpu_cif_stamps_adapter import field, run, segments
from test_gpu_pipeline import make_file, shape_vad_weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V = 300
BEAMS = (8, 16)                                  # glob_beam, lat_beam: width min(8, 8), beam min(16, 16)


def tagged(lines, tag):
    return segments([l[len(tag) + 1:] for l in lines if l.startswith(tag + "_seg ")])


def pick_hotword(asr, pcm, segs):
    """(segment index, [a, b], score): the runner-up candidates of two adjacent rows of a segment, not adjacent in any greedy text,
    and an integer score above both gaps to the best candidates (from the returned log-probabilities), so that taking the word gains
    at every one of its rows."""
    greedy = [ids for _, _, ids in segs]
    best = None
    for i, (s, e, ids) in enumerate(segs):
        if len(ids) < 3:
            continue
        r = asr.forward_ids([pcm[s:e]], nbest=2)
        cid, lp = r["nbest_ids"][0], r["nbest_logp"][0]
        for t in range(len(ids) - 1):
            a, b = int(cid[t, 1]), int(cid[t + 1, 1])
            gap = max(float(lp[t, 0] - lp[t, 1]), float(lp[t + 1, 0] - lp[t + 1, 1]))
            if a >= 1 and b >= 1 and a != b and not any(g[j:j + 2] == [a, b] for g in greedy for j in range(len(g) - 1)):
                if best is None or gap < best[0]:
                    best = (gap, i, [a, b])
    assert best is not None, "no usable pair of runner-up candidates: choose another seed"
    return best[1], best[2], int(math.ceil(best[0])) + 1


@pytest.fixture(scope="module")
def offline(pkg, weights_mod, tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    tmp = tmp_path_factory.mktemp("pfbias")
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
    seg_i, word, score = pick_hotword(asr, f32, segs)
    text = "".join(tokens[t] for t in word)
    # nbest 8 and CIF stamps on: the passes with a decoder handle carry confidences and stamps
    lines = run(base + ["8", "1", str(BEAMS[0]), str(BEAMS[1]), text, str(score)])
    yield dict(pkg=pkg, asr=asr, f32=f32, tokens=tokens, segs=segs, seg_i=seg_i, word=word, score=score, text=text, lines=lines)
    asr.close()


def test_a_paraformer_stream_gets_a_decoder_and_without_hotwords_nothing_changes(offline):
    """FunASRCtcDecoderInit is non-null now; with no hotword loaded the text, ids, stamps and confidences equal those of
    dec_handle = nullptr with the same settings (the harness's nbest and cif_stamps passes)."""
    L = offline["lines"]
    assert field(L, "dec_handle") == "1"
    assert tagged(L, "dec") == offline["segs"] == segments(L)
    assert field(L, "dec_text") == field(L, "text") == field(L, "nbest_text") == field(L, "cif_text")
    assert field(L, "dec_stamp") == field(L, "cif_stamp") != ""
    assert field(L, "dec_confidence") == field(L, "confidence") != ""


def test_hotwords_from_text_bias_the_text_and_ids_are_hypothesis_0(offline):
    o, L = offline, offline["lines"]
    pkg, asr, tokens = o["pkg"], o["asr"], o["tokens"]
    assert field(L, "hw_loaded") == "1"
    graph = pkg.ContextGraph([o["word"]], [[float(o["score"])] * 2], V)
    got = tagged(L, "hw")
    assert [(s, e) for s, e, _ in got] == [(s, e) for s, e, _ in o["segs"]]
    want_conf, changed = [], 0
    for (s, e, ids), (_, _, plain) in zip(got, o["segs"]):
        r = asr.forward_bias([o["f32"][s:e]], [(min(BEAMS[0], 8), min(BEAMS[1], 16), 1, graph)], nbest=8)
        want = r["hyps"][0][0][0].tolist() if r["hyps"][0] else []
        assert ids == want, (s, e)
        assert len(ids) == len(plain)                                      # tokens are replaced position by position
        changed += int(ids != plain)
        for t, tok in enumerate(ids):                                      # exp of the CHOSEN candidate's log-probability
            col = r["nbest_ids"][0, t].tolist().index(tok)
            want_conf.append(np.exp(r["nbest_logp"][0, t, col]))
    assert changed >= 1
    word = o["word"]
    has = lambda seq: any(seq[j:j + 2] == word for j in range(len(seq) - 1))
    assert has(got[o["seg_i"]][2]) and not any(has(p) for _, _, p in o["segs"])
    text = field(L, "hw_text")
    assert text == "".join(tokens[i] for _, _, ids in got for i in ids) and o["text"] in text and o["text"] not in field(L, "text")
    conf = np.asarray([float(x) for x in field(L, "hw_confidence").split()], np.float32)
    want_conf = np.asarray(want_conf, np.float32)
    assert conf.shape == want_conf.shape and len(conf) == len(text)
    rel = float(np.max(np.abs(conf - want_conf) / want_conf))
    print(f"{len(conf)} confidences, max rel diff {rel:.3e} (bound 2^-22: two float exp implementations)")
    assert rel <= 2.0 ** -22
    graph.close()


def test_cif_stamps_count_the_biased_tokens(offline):
    L = offline["lines"]
    text = field(L, "hw_text")
    pairs = json.loads(field(L, "hw_stamp"))
    assert len(pairs) == len(text) > 0 and all(b <= e for b, e in pairs)


def test_two_pass_second_pass_takes_the_handle(pkg, weights_mod, tmp_path):
    """FunTpassInferBuffer with a decoder handle: with no hotword loaded every line is the line without a handle; with hotwords the
    second-pass ids change position by position (their count per segment stays), only into hotword tokens, and the text follows."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    pcm = make_file(np.random.default_rng(21))[:16000 * 12]
    s16 = np.clip(np.round(pcm * 32768.0), -32768, 32767).astype("<i2")
    vman, vblob = shape_vad_weights(*weights_mod.synth_vad_weights())
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=V)
    aman, ablob = weights_mod.synth_weights(cfg, seed=31)
    oman, oblob = weights_mod.synth_weights(cfg, seed=77)
    dirs = {k: tmp_path / k for k in ("asr", "online", "vad")}
    for d in dirs.values():
        d.mkdir()
    weights_mod.save(str(dirs["asr"] / "model.pfhip"), aman, ablob)
    weights_mod.save(str(dirs["online"] / "model.pfhip"), oman, oblob)
    weights_mod.save(str(dirs["vad"] / "vad.pfhip"), vman, vblob)
    tokens = [chr(0x4E00 + i) for i in range(V)]
    with open(dirs["asr"] / "tokens.json", "w") as f:
        json.dump(tokens, f)
    s16.tofile(tmp_path / "stream.pcm")
    exe = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "tpass_infer")
    base = [exe, str(dirs["asr"]), str(dirs["online"]), str(dirs["vad"]), str(tmp_path / "stream.pcm"), "9600", "2"]
    tail = ["-", "16000", "0", "0", "auto", "1", "0", str(BEAMS[0]), str(BEAMS[1])]
    calls = lambda lines: [l.split(" | ") for l in lines if l.startswith("call ")]
    off = calls(run(base))
    none = run(base + tail)                                                # a handle, no hotword
    assert none[0] == "dec_handle 1 hw_loaded 0"
    assert [c[:4] for c in calls(none)] == [c[:4] for c in off]
    plain_ids = [[int(x) for x in c[4].split()[1:]] for c in calls(none)]
    texts = [c[2][len("tpass "):].strip() for c in off]
    assert sum(1 for t in texts if t) >= 2
    for ids, t in zip(plain_ids, texts):
        assert "".join(tokens[i] for i in ids).endswith(t)                 # (a call that closes two segments keeps the last text)
    # Hotwords that must change the text whatever the segments are: every token the plain second-pass texts lack (id 0, the graph's
    # escape label, left out) as a one-token hotword with a score no gap of this model reaches.  A row then takes the best of its 8
    # candidates that is such a token, and keeps its own only where all 8 occur in the plain texts.
    seen = {i for ids in plain_ids for i in ids}
    hotset = [i for i in range(1, V) if i not in seen]
    args = [x for i in hotset for x in (tokens[i], "40")]
    hot = run(base + tail + args)
    assert hot[0] == f"dec_handle 1 hw_loaded {len(hotset)}"
    hot_calls = calls(hot)
    assert len(hot_calls) == len(off) and [c[1] for c in hot_calls] == [c[1] for c in off]       # the online pass does not change
    hot_ids = [[int(x) for x in c[4].split()[1:]] for c in hot_calls]
    assert [len(x) for x in hot_ids] == [len(x) for x in plain_ids]        # position by position: the counts stay
    changed = [(a, b) for x, y in zip(hot_ids, plain_ids) for a, b in zip(x, y) if a != b]
    assert changed and all(a in hotset for a, _ in changed)
    for ids, c in zip(hot_ids, hot_calls):
        assert "".join(tokens[i] for i in ids).endswith(c[2][len("tpass "):].strip())
