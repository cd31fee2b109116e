"""GPU: SenseVoiceSmall as the second pass of the 2-pass flow, through `tpass_infer` on directories in the reference's layout:
FunTpassInit picks SenseVoiceSmallHip because the offline directory is named `SenseVoiceSmall_synth` (tpass-stream.cpp:44-50) and
makes the NINE-argument InitAsr on it (the small online Paraformer's model.onnx / decoder.onnx, the ONLINE directory's am.mvn for
both models, :72-77); FunTpassOnlineInit builds ParaformerOnlineHip(model, chunk_size, MODEL_SVS); FunTpassInferBuffer routes the
second pass by model type with its trailing svs_lang / svs_itn and leaves the text without punctuation.

The flow is driven as tests/test_gpu_ref_layout.py::test_tpass_stream_calls_on_reference_directories drives it (same audio cutter,
same 600-ms messages).  Streaming ids per call equal the streaming oracle's; every closed segment's second-pass ids equal, exactly,
SenseVoiceHip.forward of that segment (one library, one forward); the text is sensevoice_ref.ctc_text of those ids; with
FunTpassSetCtcStamps every stamp pair is the forward's span times 60 ms plus the segment's start."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ref_layout as RL
import sensevoice_ref as R
from oracle import audio_split as A
from oracle import paraformer as P
from oracle import paraformer_online as PO
from test_gpu_pipeline import make_file, shape_vad_weights
from test_gpu_sensevoice_adapter import vocabulary

pytestmark = pytest.mark.gpu
FRAME_MS = 60


@pytest.fixture(scope="module")
def setup(pkg, weights_mod, tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    conv = importlib.import_module(pkg.__name__ + ".convert")
    tmp = tmp_path_factory.mktemp("svs_tpass")
    pcm = make_file(np.random.default_rng(21))[:16000 * 30]
    s16 = np.clip(np.round(pcm * 32768.0), -32768, 32767).astype("<i2")
    vman, vblob = shape_vad_weights(*weights_mod.synth_vad_weights())
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=300)
    oman, oblob = weights_mod.synth_weights(cfg, seed=32)
    sman, sblob = weights_mod.synth_svs_weights()
    vocab = vocabulary(sman["config"]["vocab"])
    svs_dir = tmp / "SenseVoiceSmall_synth"
    R.write_model_dir(str(svs_dir), conv, sman, sblob, vocab_tokens=vocab)
    RL.write_asr_dir(str(tmp / "online"), conv, oman, oblob, cfg, online=True, vocab_tokens=[])
    os.remove(tmp / "online" / "tokens.json")                   # no online vocabulary: the harness prints the streaming ids
    RL.write_vad_dir(str(tmp / "vad"), conv, vman, vblob)
    s16.tofile(tmp / "stream.pcm")
    # the mirror of the second pass: the same files, the ONLINE directory's am.mvn as the nine-argument InitAsr passes it
    mirror = pkg.SenseVoiceHip().InitAsr(str(svs_dir / "model.onnx"), str(tmp / "online" / "am.mvn"), str(svs_dir / "config.yaml"))
    vad = pkg.FsmnVadHip().InitVad((vman, vblob))
    exe = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "tpass_infer")
    yield dict(tmp=tmp, s16=s16, vocab=vocab, mirror=mirror, vad=vad, online=P.Weights(oman, oblob), pkg=pkg,
               cmd=[exe, str(svs_dir), str(tmp / "online"), str(tmp / "vad"), str(tmp / "stream.pcm"), "9600", "2", "-", "16000", "0", "0"])
    vad.close()
    mirror.close()


def run(s, lang, itn, stamps):
    out = subprocess.run(s["cmd"] + [lang, str(int(itn)), str(int(stamps))], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return [l.split(" | ") for l in out.stdout.splitlines() if l.startswith("call ")]


def field(parts, name):
    for p in parts:
        if p == name or p.startswith(name + " "):
            return p[len(name) + 1:]
    raise AssertionError((name, parts))


def check_flow(s, got, lang, itn, stamps):
    """The oracle's cutter and streaming model beside the harness's lines; the second pass against the Python mirror."""
    pkg, f32 = s["pkg"], (s["s16"].astype(np.float32) / 32768.0).astype(np.float32)
    vad_on = pkg.FsmnVadOnlineHip(s["vad"], 800, 60000, 0.9)
    online, audio = PO.ParaformerOnline(s["online"]), A.TpassAudio()
    n_tpass = n_online = n_pairs = 0
    for j, off in enumerate(range(0, len(f32), 9600)):
        last = off + 9600 >= len(f32)
        audio.LoadPcmwavOnline(f32[off:off + 9600])
        audio.Split(lambda w, fin: vad_on.Infer(w, fin), 9600, last, A.ASR_TWO_PASS)
        want_online = []
        while True:
            fr = audio.FetchChunck()
            if fr is None:
                break
            want_online += [int(i) for i in online.Forward(fr["data"], fr["is_final"])]
        assert [int(x) for x in field(got[j], "online").split()] == want_online, j
        n_online += len(want_online)
        want_ids, want_text, want_pairs = [], "", []
        while True:
            fr = audio.FetchTpass()
            if fr is None:
                break
            ref = s["mirror"].forward([np.asarray(fr["data"], np.float32)], lang=lang, itn=itn, want_spans=True)
            ids = ref["ids"][0].tolist()
            text = R.ctc_text(ids, s["vocab"]) if int(ref["frame_len"][0]) else ""
            if text == "":
                continue                                         # the flow skips an empty second pass (funasrruntime.cpp:588)
            n_tpass += 1
            want_ids += ids
            want_text = text                                     # tpass_msg is the last closed segment's, as in the reference
            if np.isfinite(ref["span_score"][0]):
                want_pairs += [[(int(b) - 4) * FRAME_MS + fr["global_start"], (int(e) - 4) * FRAME_MS + fr["global_start"]]
                               for b, e in zip(ref["span_begin"][0], ref["span_end"][0])]
        assert [int(x) for x in field(got[j], "tpass_ids").split()] == want_ids, j
        assert field(got[j], "tpass") == want_text, (j, field(got[j], "tpass"), want_text)
        have_pairs = [[int(a), int(b)] for a, b in re.findall(r"\[(-?\d+),(-?\d+)\]", field(got[j], "stamp"))]
        assert have_pairs == (want_pairs if stamps else []), (j, have_pairs, want_pairs)
        n_pairs += len(have_pairs)
        if last:
            audio.ResetIndex()
    vad_on.close()
    assert len(got) == j + 1 and n_tpass >= 3 and n_online > 20
    return n_pairs


def test_second_pass_is_sensevoice_with_stamps(setup):
    got = run(setup, "en", True, True)
    n_pairs = check_flow(setup, got, "en", True, True)
    assert n_pairs > 10                                          # there were stamps to compare


def test_svs_lang_and_itn_reach_the_second_pass(setup):
    """The same flow with another svs_lang / svs_itn (and no stamps): still the mirror's ids and text, and not the first run's."""
    a = run(setup, "en", True, False)
    b = run(setup, "zh", False, False)
    check_flow(setup, b, "zh", False, False)
    assert not any(re.search(r"\d", field(l, "stamp")) for l in a + b)                # the switch is off: no stamps
    assert [field(l, "tpass_ids") for l in a] != [field(l, "tpass_ids") for l in b]
    assert [field(l, "tpass") for l in a] != [field(l, "tpass") for l in b]
    assert [field(l, "online") for l in a] == [field(l, "online") for l in b]      # the first pass does not depend on them
