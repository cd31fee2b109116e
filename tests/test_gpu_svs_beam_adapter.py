"""GPU: the per-connection decoder object CtcPrefixDecoderHip (csrc/host/ctc_prefix_decoder_hip.{h,cpp}) behind the C++ adapter and the
stand-alone handle API, through the `svs_infer` harness on the directory and utterances of test_gpu_sensevoice_adapter.py.

With a CtcPrefixDecoderHip as decoder handle SenseVoiceSmallHip runs the device search: the best ids must equal, exactly, those of the
Python mirror's forward(beam=..., graph=...) on the same samples (one library), where the mirror's graph is built here from the
hotword TEXT by a restatement of the reference's greedy longest match (context_graph.cpp:120-159) and weight rule (:76-77); the text
must be the pieces concatenated with the word-start mark turned into a space, plus the trailing-space rule on the tags of rows 0 and
3 (sensevoice-small.cpp:413-436).  With the harness's stub Decoder the hand-off of full rows happens exactly as before."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import sensevoice_ref as R
from conftest import synth_pcm
from test_gpu_sensevoice_adapter import vocabulary

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ENV = dict(os.environ, PFHIP_WARMUP_SECONDS="0")


@pytest.fixture(scope="module")
def setup(pkg, tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    wt = importlib.import_module("asr_2pass_amd.weights")
    conv = importlib.import_module("asr_2pass_amd.convert")
    man, blob = wt.synth_svs_weights()
    base = tmp_path_factory.mktemp("svsbeam")
    d = base / "SenseVoiceSmall_synth"
    vocab = vocabulary(man["config"]["vocab"])
    R.write_model_dir(str(d), conv, man, blob, vocab_tokens=vocab)
    utts = []
    for i, seconds in enumerate((1.0, 0.02, 2.5)):
        x = synth_pcm(30 + i, int(seconds * 16000), np.random.default_rng(900 + i))
        s16 = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
        s16.tofile(str(d / f"utt{i}.pcm"))
        utts.append(s16)
    model = pkg.SenseVoiceHip().InitAsr((man, blob), device=0)
    yield dict(dir=d, vocab=vocab, utts=utts, model=model, pkg=pkg,
               exe=os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "svs_infer"))
    model.close()


def text_to_ids(text, vocab):
    """SplitUTF8StringToWords restated: greedy longest match over code points, alphabetic words with the word-start mark, spaces
    skipped; (ids, pieces, every piece known)."""
    index = {}
    for i, t in enumerate(vocab):
        index.setdefault(t, i)
    chars, ids, words, ok, start = list(text.strip()), [], [], True, 0
    while start < len(chars):
        for end in range(len(chars), start, -1):
            word = "".join(chars[start:end])
            if word == " ":
                start = end
                break
            if word.isascii() and word.isalpha():
                word = R.WORD_START + word
            if word in index:
                ids.append(index[word]); words.append(word)
                start = end
                break
            if end == start + 1:
                start += 1
                ok = False
                break
    return ids, words, ok


def graph_of(s, hotwords):
    """The mirror's ContextGraph for {text: score}: a token weighs score x the code points of its piece; unknown pieces skip the word."""
    words, weights = [], []
    for text, score in hotwords.items():
        ids, pieces, ok = text_to_ids(text, s["vocab"])
        if ok and ids:
            words.append(ids); weights.append([float(score) * len(p) for p in pieces])
    return (s["pkg"].ContextGraph(words, weights, len(s["vocab"])) if words else None), len(words)


def expected_text(s, ids, frame_ids):
    text = "".join(s["vocab"][i] for i in ids).replace(R.WORD_START, " ")
    lang, itn = s["vocab"][frame_ids[0]], s["vocab"][frame_ids[3]]
    if itn == "<|withitn|>":
        return text + (" " if lang == "<|en|>" else "")
    return text + " "


def parse(stdout):
    out = {}
    for line in stdout.splitlines():
        if " text [" in line:
            key, _, val = line.partition(" text [")
            out[key + " text"] = val[:-1]
        elif " stamp [" in line:
            key, _, val = line.partition(" stamp [")
            out[key + " stamp"] = val[:-1]
        elif " : " in line or line.endswith(" :"):
            key, _, val = line.partition(" :")
            out[key] = [int(x) for x in val.split()]
        elif line.startswith("hotwords loaded "):
            out["loaded"] = int(line.split()[-1])
    return out


def run_beam(s, lang, itn, hotwords, beams=(3, 3), stamps=False):
    cmd = [s["exe"]] + (["--ctc-stamps"] if stamps else []) + ["--beam", str(s["dir"] / "model.onnx"), str(s["dir"] / "tokens.json"), lang,
                                                               str(int(itn)), str(beams[0]), str(beams[1])]
    for text, score in hotwords.items():
        cmd += ["--hotword", text, str(score)]
    cmd += [str(s["dir"] / f"utt{i}.pcm") for i in range(3)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return parse(r.stdout), r.stdout


def hotwords_for(s):
    """A hotword spelt from three neighbouring tokens of the plain search's best hypothesis that text can name (no word-start piece:
    "w12" is not alphabetic, so the reference's rule could not find it), and one with a piece outside the vocabulary."""
    plain = s["model"].forward(s["utts"], lang="en", itn=True, beam=(3, 3), nbest=1)
    best = plain["beam_ids"][2][0].tolist()
    run3 = next(best[i:i + n] for n in (3, 2, 1) for i in range(len(best) - n + 1) if all(t % 3 != 0 for t in best[i:i + n]))
    return {"".join(s["vocab"][t] for t in run3): 5, "zz9 top": 4}, run3


@pytest.mark.parametrize("lang,itn", [("en", True), ("zh", False)])
def test_device_search_text_and_ids(setup, lang, itn):
    s = setup
    got, raw = run_beam(s, lang, itn, {})
    ref = s["model"].forward(s["utts"], lang=lang, itn=itn, beam=(3, 3), nbest=1)
    assert got["loaded"] == 0
    for b in range(3):
        want = ref["beam_ids"][b][0].tolist() if ref["beam_n_hyp"][b] else []
        assert got[f"utt {b} search ids"] == want, raw
        assert got[f"utt {b} greedy ids"] == ref["ids"][b].tolist()
        text = expected_text(s, want, ref["frame_ids"][b].tolist()) if ref["frame_len"][b] else ""
        assert got[f"utt {b} text"] == text, (b, got[f"utt {b} text"], text)
        assert got[f"unloaded utt {b} search ids"] == want
    assert len(got["utt 2 search ids"]) > 4 and got["utt 1 search ids"] == [] and got["utt 1 text"] == ""


def test_hotwords_from_text_reach_the_device(setup):
    s = setup
    hot, run3 = hotwords_for(s)
    assert text_to_ids(next(iter(hot)), s["vocab"])[0] == run3 and not text_to_ids("zz9 top", s["vocab"])[2]
    graph, n = graph_of(s, hot)
    assert n == 1
    got, raw = run_beam(s, "en", True, hot)
    assert got["loaded"] == 1, raw                       # the hotword with an unknown piece is skipped
    ref = s["model"].forward(s["utts"], lang="en", itn=True, beam=(3, 3), nbest=1, graph=graph)
    plain = s["model"].forward(s["utts"], lang="en", itn=True, beam=(3, 3), nbest=1)
    assert ref["beam_ctx_score"][2][0] > 0               # the graph counted in the mirror ...
    for b in (0, 2):
        want = ref["beam_ids"][b][0].tolist()
        assert got[f"utt {b} search ids"] == want, raw   # ... and the adapter's graph, made from the text, gives the same search
        assert got[f"utt {b} text"] == expected_text(s, want, ref["frame_ids"][b].tolist())
        assert got[f"unloaded utt {b} search ids"] == plain["beam_ids"][b][0].tolist()      # UnloadHwsRes: the plain search again
    graph.close()


def test_spans_of_the_search_ids(setup):
    """SetCtcTimestamps on: such a call gets spans — those of pfhip_svs_align on the best ids, 60 ms a row."""
    s = setup
    got, raw = run_beam(s, "en", True, {}, stamps=True)
    ref = s["model"].forward(s["utts"], lang="en", itn=True, beam=(3, 3), nbest=1)
    al = s["model"].align([h[0] if len(h) else np.zeros(0, np.int32) for h in ref["beam_ids"]])
    for b in (0, 2):
        want = []
        for tb, te in zip(al["begin"][b].tolist(), al["end"][b].tolist()):
            want += [(tb - 4) * 60, (te - 4) * 60]
        assert got[f"utt {b} stamps"] == want, raw
    assert len(got["utt 2 stamps"]) == 2 * len(got["utt 2 search ids"]) > 8 and got["utt 1 stamps"] == []


def test_handle_api_decoder(setup):
    """FunASRCtcDecoderInit -> FunCtcDecoderLoadHwsRes -> FunOfflineInferBuffer(dec_handle) -> FunCtcDecoderUninit."""
    s = setup
    hot, _ = hotwords_for(s)
    graph, _ = graph_of(s, hot)
    cmd = [s["exe"], "--ctc-stamps", "--beam-handle-api", str(s["dir"]), "en", "1", "3", "3"]
    for text, score in hot.items():
        cmd += ["--hotword", text, str(score)]
    r = subprocess.run(cmd + [str(s["dir"] / "utt2.pcm")], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = parse(r.stdout)
    ref = s["model"].forward([s["utts"][2]], lang="en", itn=True, beam=(3, 3), nbest=1, graph=graph)
    ids = ref["beam_ids"][0][0].tolist()
    assert got["loaded"] == 1
    assert got["handle text"] == expected_text(s, ids, ref["frame_ids"][0].tolist()), r.stdout
    assert got["handle stamp"].count("[") == len(ids) + 1        # one [b,e] pair per token of the search's text
    graph.close()


def test_any_other_decoder_keeps_the_hand_off(setup):
    """The harness's stub Decoder is no CtcPrefixDecoderHip: it is handed the full log-prob rows of every utterance, restarted between
    items and finalised when input_finished — what tests/test_gpu_sensevoice_adapter.py holds for the hand-off."""
    s = setup
    r = subprocess.run([s["exe"], "--decoder", str(s["dir"] / "model.onnx")] + [str(s["dir"] / f"utt{i}.pcm") for i in range(3)],
                       capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ref = s["model"].forward(s["utts"], lang="auto", itn=False)
    searches = [ln for ln in r.stdout.splitlines() if ln.startswith("search ")]
    V = s["model"].cfg["vocab"]
    assert len(searches) == 4
    for k, ln in enumerate(searches):
        b = (0, 2)[k % 2]
        head, _, ids = ln.partition(" :")
        assert head == f"search {k} rows {int(ref['frame_len'][b])} vocab {V}"
        assert [int(x) for x in ids.split()] == ref["frame_ids"][b].tolist()
    assert "finished 0 utt 0 text [partial0]" in r.stdout and "finished 1 utt 2 text [final1]" in r.stdout
    assert "calls starts 2 ends 2 finals 2 searches 4" in r.stdout
