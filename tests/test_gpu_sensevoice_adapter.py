"""GPU: the C++ adapter SenseVoiceSmallHip (csrc/host/sensevoice_hip.{h,cpp}) through the `svs_infer` harness: the five-argument
InitAsr on a directory in the reference's file layout (a synthetic model.onnx with the upstream names, am.mvn, config.yaml,
tokens.json; named as the reference's factory expects, offline-stream.cpp:50-56) and on a container, one packed ForwardPcm16 over
three files and one Forward on floats.  Ids and frames must equal, exactly, what the Python mirror gets from the
same 16-bit samples (one library, one forward); the text must equal the restated CTCSearch (tests/sensevoice_ref.py) of those ids."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import sensevoice_ref as R
from conftest import synth_pcm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def vocabulary(n):
    """<blank>, language / emotion / event / ITN tags where the synthetic model may or may not put them, word pieces with and
    without the word-start marker, CJK characters."""
    v = ["<blank>", "<|zh|>", "<|en|>", "<|NEUTRAL|>", "<|Speech|>", "<|withitn|>", "<|woitn|>"]
    while len(v) < n:
        i = len(v)
        v.append((R.WORD_START + "w%d" % i) if i % 3 == 0 else ("p%d" % i if i % 3 == 1 else chr(0x4E00 + i)))
    return v


@pytest.fixture(scope="module")
def setup(pkg, tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    wt = importlib.import_module("asr_2pass_amd.weights")
    conv = importlib.import_module("asr_2pass_amd.convert")
    man, blob = wt.synth_svs_weights()
    base = tmp_path_factory.mktemp("svs")
    d = base / "SenseVoiceSmall_synth"
    vocab = vocabulary(man["config"]["vocab"])
    R.write_model_dir(str(d), conv, man, blob, vocab_tokens=vocab)      # model.onnx: the C++ reader converts it (and caches beside it)
    (base / "container").mkdir()
    wt.save(str(base / "container" / "svs.pfhip"), man, blob)           # svs.pfhip.bin / .json
    utts = []
    for i, seconds in enumerate((1.0, 0.02, 2.5)):
        x = synth_pcm(30 + i, int(seconds * 16000), np.random.default_rng(900 + i))
        s16 = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
        s16.tofile(str(d / f"utt{i}.pcm"))
        utts.append(s16)
    model = pkg.SenseVoiceHip().InitAsr((man, blob), device=0)
    yield dict(dir=d, container=base / "container" / "svs.pfhip.bin", vocab=vocab, utts=utts, model=model, exe=os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "svs_infer"))
    model.close()


def run(s, am_model, tokens, lang, itn):
    env = dict(os.environ, PFHIP_WARMUP_SECONDS="0")
    cmd = [s["exe"], str(am_model), tokens, lang, str(int(itn))] + [str(s["dir"] / f"utt{i}.pcm") for i in range(3)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        if " : " in line or line.endswith(" :"):
            key, _, val = line.partition(" :")
            out[key] = [int(x) for x in val.split()]
        elif " text [" in line:
            key, _, val = line.partition(" text [")
            out[key + " text"] = val[:-1]
    return out, r.stdout


@pytest.mark.parametrize("lang,itn,name", [("en", True, "model.onnx"), ("zh", False, "container")])
def test_adapter_equals_the_python_mirror(setup, lang, itn, name):
    s = setup
    assert os.path.getsize(s["dir"] / "model.onnx") > 1 << 20                                   # a real ONNX file is what gets read
    got, raw = run(s, s["dir"] / name if name == "model.onnx" else s["container"], str(s["dir"] / "tokens.json"), lang, itn)
    ref = s["model"].forward(s["utts"], lang=lang, itn=itn)
    for b in range(3):
        assert got[f"utt {b} ids"] == ref["ids"][b].tolist(), raw
        assert got[f"utt {b} frames"] == ref["tok_frame"][b].tolist()
        want = R.ctc_text(ref["ids"][b].tolist(), s["vocab"]) if ref["frame_len"][b] else ""      # no frame: "" (sensevoice-small.cpp:584-587)
        assert got[f"utt {b} text"] == want, (b, got[f"utt {b} text"], want)
    assert len(got["utt 0 ids"]) > 4 and got["utt 1 ids"] == []
    assert got["alone ids"] == got["utt 0 ids"] and got["alone text"] == got["utt 0 text"]      # Forward on floats, one utterance
    assert raw.count("confidence_ok 1") == 3


def test_without_a_vocabulary_the_ids_are_the_text(setup):
    s = setup
    got, _ = run(s, s["container"], "-", "auto", False)
    assert got["utt 0 text"] == " ".join(str(i) for i in got["utt 0 ids"][4:])


def test_handle_api_routes_by_the_directory_name(setup):
    """FunOfflineInit on a directory whose name contains MODEL_SVS builds SenseVoiceSmallHip (offline-stream.cpp:50-56) and
    FunOfflineInferBuffer passes its two trailing parameters svs_lang / svs_itn on (funasrruntime.cpp:265-266): without a VAD the
    buffer is one segment, whose ids and text are those of the Python mirror for the same samples."""
    s = setup
    env = dict(os.environ, PFHIP_WARMUP_SECONDS="0")
    r = subprocess.run([s["exe"], "--handle-api", str(s["dir"]), "en", "1", str(s["dir"] / "utt2.pcm")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ref = s["model"].forward([s["utts"][2]], lang="en", itn=True)
    seg = [ln for ln in r.stdout.splitlines() if ln.startswith("seg ")]
    assert len(seg) == 1 and seg[0].startswith(f"seg 0 {len(s['utts'][2])} :")
    assert [int(x) for x in seg[0].partition(" :")[2].split()] == ref["ids"][0].tolist()
    text = [ln for ln in r.stdout.splitlines() if ln.startswith("handle text [")][0][len("handle text ["):-1]
    assert text == R.ctc_text(ref["ids"][0].tolist(), s["vocab"])
    other = subprocess.run([s["exe"], "--handle-api", str(s["dir"]), "zh", "0", str(s["dir"] / "utt2.pcm")], capture_output=True,
                           text=True, timeout=120, env=env)
    assert other.returncode == 0 and other.stdout != r.stdout            # the two parameters reach the model


def test_decoder_handle_gets_every_utterances_rows(setup):
    """With a decoder handle the full log-prob rows of every utterance go to Decoder::Search (the search itself is not part of this
    path): a stub records them.  Utterance 1 has no frame: it is skipped, its text is "", and the rows of utterance 2 start where
    utterance 0's end.  Between items the decoder is restarted; FinalizeDecode is called only when input_finished."""
    s = setup
    env = dict(os.environ, PFHIP_WARMUP_SECONDS="0")
    r = subprocess.run([s["exe"], "--decoder", str(s["container"])] + [str(s["dir"] / f"utt{i}.pcm") for i in range(3)], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ref = s["model"].forward(s["utts"], lang="auto", itn=False)
    searches = [ln for ln in r.stdout.splitlines() if ln.startswith("search ")]
    assert len(searches) == 4                                  # two calls x the two utterances that have rows
    V = s["model"].cfg["vocab"]
    for k, ln in enumerate(searches):
        b = (0, 2)[k % 2]
        head, _, ids = ln.partition(" :")
        assert head == f"search {k} rows {int(ref['frame_len'][b])} vocab {V}"
        assert [int(x) for x in ids.split()] == ref["frame_ids"][b].tolist()      # the arg-max of the rows handed over: that utterance's
    text = {ln.split(" text ")[0]: ln.split(" text ")[1] for ln in r.stdout.splitlines() if ln.startswith("finished ")}
    assert text["finished 0 utt 0"] == "[partial0]" and text["finished 0 utt 1"] == "[]" and text["finished 0 utt 2"] == "[partial1]"
    assert text["finished 1 utt 0"] == "[final0]" and text["finished 1 utt 1"] == "[]" and text["finished 1 utt 2"] == "[final1]"
    assert "calls starts 2 ends 2 finals 2 searches 4" in r.stdout           # one restart per call, in front of the second item with rows


def test_create_from_files_recognises_the_kind(setup, pkg):
    """pfhip_create_from_files on model.onnx + am.mvn + config.yaml gives a SenseVoice handle whose forward equals the container's."""
    s = setup
    d = s["dir"]
    m = pkg.SenseVoiceHip().InitAsr(str(d / "model.onnx"), str(d / "am.mvn"), str(d / "config.yaml"), device=0)
    try:
        assert m._lib.pfhip_is_ctc(m._h) == 1 and m.cfg["kind"] == "sensevoice" and m.cfg["tp_layers"] == 2
        a, b = m.forward(s["utts"], lang="en", itn=True), s["model"].forward(s["utts"], lang="en", itn=True)
        for x, y in zip(a["frame_ids"], b["frame_ids"]):
            assert x.tolist() == y.tolist()
        for x, y in zip(a["frame_logp"], b["frame_logp"]):
            assert np.array_equal(x, y)                       # the same weights, bit for bit, through the same kernels
    finally:
        m.close()
