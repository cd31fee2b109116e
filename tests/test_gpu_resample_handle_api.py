"""GPU: the handle API at other sample rates.  FunOfflineInferBuffer and FunTpassInferBuffer with `sampling_rate` != 16000
resample as Audio::LoadPcmwav / LoadPcmwavOnline do (onnxruntime/src/audio.cpp:787-857 -> WavResample :259-284): the whole
buffer once (offline), each message on its own with flush (2-pass).  Compared with the Python flows of
tests/test_gpu_pipeline.py fed with PCM resampled by the NumPy restatement (tests/resample_ref.py)."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import resample_ref as R
from conftest import synth_pcm
from test_gpu_pipeline import shape_vad_weights

pytestmark = pytest.mark.gpu


def make_file_at(fs, rng, secs=(4.0, 7.5, 2.2, 11.0, 5.3)):
    """The pipeline tests' speech-like bursts and 1.2-s digital silences, as s16 at rate fs."""
    parts = []
    for i, sec in enumerate(secs):
        parts.append(synth_pcm(i, int(sec * fs), rng))
        parts.append(np.zeros(int(1.2 * fs), np.float32))
    pcm = np.concatenate(parts)
    return np.clip(np.round(pcm * 32768.0), -32768, 32767).astype("<i2")


@pytest.mark.parametrize("fs", [8000, 44100])
def test_offline_handle_api_at_other_rates(pkg, weights_mod, tmp_path, fs):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    pipeline = importlib.import_module("asr_2pass_amd.pipeline")
    rng = np.random.default_rng(fs)
    s16 = make_file_at(fs, rng)
    pcm = R.resample(s16.astype(np.float32) / np.float32(32768.0), fs)       # LoadPcmwav + WavResample
    vman, vblob = shape_vad_weights(*weights_mod.synth_vad_weights())
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=300, timestamp=1)
    aman, ablob = weights_mod.synth_weights(cfg)
    mdir, vdir = tmp_path / "asr", tmp_path / "vad"
    mdir.mkdir(); vdir.mkdir()
    weights_mod.save(str(mdir / "model.pfhip"), aman, ablob)
    weights_mod.save(str(vdir / "vad.pfhip"), vman, vblob)
    with open(mdir / "tokens.json", "w") as f:
        json.dump([f"<{i}>" for i in range(300)], f)
    s16.tofile(tmp_path / "long.pcm")
    exe = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "offline_infer")
    vad = pkg.FsmnVadHip().InitVad((vman, vblob))
    asr = pkg.ParaformerHip().InitAsr((aman, ablob))
    seg = pkg.E2EVadModelHost()
    ids, frames = pipeline.infer_buffer(pcm, asr, vad, seg, batch_size=4, vad_max_len=60000)
    assert len(frames) >= 3
    out = subprocess.run([exe, str(mdir), str(vdir), str(tmp_path / "long.pcm"), "4", "4", "2", "-", str(fs)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr             # 4 threads re-run the file: 0 results differ (else exit 3)
    lines = out.stdout.splitlines()
    segs = [l for l in lines if l.startswith("seg ")]
    assert len(segs) == len(frames)
    for l, (s, e), want in zip(segs, frames, ids):
        head, _, tail = l.partition(":")
        assert [int(x) for x in head.split()[1:3]] == [s, e]                # model-rate sample indices
        assert [int(x) for x in tail.split()] == list(want)
    text = [l for l in lines if l.startswith("text ")][0][5:]
    assert text == "".join(" ".join(f"<{i}>" for i in seg_ids) for seg_ids in ids)
    stamp = [l for l in lines if l.startswith("stamp ")][0][6:]
    pairs = json.loads(stamp) if stamp else []
    assert len(pairs) == sum(len(x) for x in ids)
    assert all(b <= e for b, e in pairs) and pairs == sorted(pairs)
    assert pairs[-1][1] <= 1000 * len(pcm) / 16000 + 1                      # stamps on the model-rate time axis
    vad.close(); asr.close(); seg.close()


def test_offline_handle_api_refuses_unsupported_rate(pkg, weights_mod, tmp_path):
    cfg = weights_mod.small_config(enc_layers=1, dec_layers=1, vocab=300)
    aman, ablob = weights_mod.synth_weights(cfg)
    mdir = tmp_path / "asr"
    mdir.mkdir()
    weights_mod.save(str(mdir / "model.pfhip"), aman, ablob)
    np.zeros(16000, "<i2").tofile(tmp_path / "x.pcm")
    exe = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "offline_infer")
    out = subprocess.run([exe, str(mdir), "-", str(tmp_path / "x.pcm"), "4", "1", "1", "-", "999"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "inference failed" in out.stderr, (out.returncode, out.stderr)


def test_2pass_handle_api_at_48k_per_message(pkg, weights_mod, tmp_path):
    """800-sample messages at 48 kHz (websocket-server-2pass.cpp:135-137): each becomes 266 or 267 samples, resampled on its own
    with zero-padded edges, exactly as the reference's fresh resampler per LoadPcmwavOnline call does."""
    from oracle import audio_split as A
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    fs, step = 48000, 800
    rng = np.random.default_rng(48)
    s16 = make_file_at(fs, rng, secs=(2.5, 3.0, 1.5))[:fs * 10]
    vman, vblob = shape_vad_weights(*weights_mod.synth_vad_weights())
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=300)
    aman, ablob = weights_mod.synth_weights(cfg, seed=31)
    oman, oblob = weights_mod.synth_weights(cfg, seed=32)
    dirs = {k: tmp_path / k for k in ("asr", "online", "vad")}
    for d in dirs.values():
        d.mkdir()
    weights_mod.save(str(dirs["asr"] / "model.pfhip"), aman, ablob)
    weights_mod.save(str(dirs["online"] / "model.pfhip"), oman, oblob)
    weights_mod.save(str(dirs["vad"] / "vad.pfhip"), vman, vblob)
    s16.tofile(tmp_path / "stream.pcm")
    exe = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "tpass_infer")
    out = subprocess.run([exe, str(dirs["asr"]), str(dirs["online"]), str(dirs["vad"]), str(tmp_path / "stream.pcm"), str(step), "2",
                          "-", str(fs)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    got = [l.split(" | ") for l in out.stdout.splitlines() if l.startswith("call ")]
    vad = pkg.FsmnVadHip().InitVad((vman, vblob))
    asr = pkg.ParaformerHip().InitAsr((aman, ablob))
    asr_on_model = pkg.ParaformerHip().InitAsr((oman, oblob))
    vad_on = pkg.FsmnVadOnlineHip(vad, 800, 60000, 0.9)
    stream = pkg.ParaformerOnlineHip(asr_on_model)
    audio = A.TpassAudio()
    f32 = (s16.astype(np.float32) / 32768.0).astype(np.float32)
    n_tpass = 0
    for j, off in enumerate(range(0, len(f32), step)):
        last = off + step >= len(f32)
        piece = R.resample(f32[off:off + step], fs)
        assert len(piece) in (266, 267) or last
        audio.LoadPcmwavOnline(piece)
        audio.Split(lambda w, fin: vad_on.Infer(w, fin), 9600, last, A.ASR_TWO_PASS)
        online_txt = ""
        while True:
            fr = audio.FetchChunck()
            if fr is None:
                break
            p = " ".join(str(i) for i in stream.Forward(fr["data"], input_finished=fr["is_final"]))
            online_txt += p + (" " if p and stream.last_path() == 2 else "")
        tpass_txt = ""
        while True:
            fr = audio.FetchTpass()
            if fr is None:
                break
            tpass_txt = " ".join(str(int(i)) for i in asr.forward_ids([fr["data"]])["ids"][0])
            n_tpass += 1
        if last:
            audio.ResetIndex()
        assert got[j][0] == f"call {j}"
        assert got[j][1] == "online " + online_txt, (j, got[j][1], online_txt)
        assert got[j][2] == "tpass " + tpass_txt, (j, got[j][2], tpass_txt)
    assert len(got) == (len(f32) + step - 1) // step and n_tpass >= 1
    for o in (vad_on, stream, vad, asr, asr_on_model):
        o.close()
