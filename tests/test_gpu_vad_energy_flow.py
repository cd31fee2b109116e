"""GPU: the long-audio flow on the energy form of the VAD.

  * pipeline.cut_split on int16 audio (never converted on the host: silence posteriors and frame energies come back from the
    device) returns the frames and index vector of the earlier logic, restated here: ForwardSil + the waveform detector fed the
    float waveform;
  * FunOfflineInferBuffer (C++ mirror, `offline_infer` harness) on 16-bit input at the model's rate, where no float copy of the
    file exists any more, gives the segments, ids and text of that flow — from four decoder threads at once, whose files the VAD
    handle scores in company (the harness exits non-zero when a thread's result differs)."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import synth_pcm
from test_gpu_pipeline import shape_vad_weights

pytestmark = pytest.mark.gpu


def make_file_s16(rng, secs=(2.0, 3.5, 1.2, 4.0)):
    parts = []
    for i, sec in enumerate(secs):
        parts.append(synth_pcm(i, int(sec * 16000), rng))
        parts.append(np.zeros(int(1.2 * 16000), np.float32))
    return np.clip(np.round(np.concatenate(parts) * 32768.0), -32768, 32767).astype("<i2")


def frames_by_the_waveform_detector(pkg, vad, f32):
    """Audio::CutSplit as pipeline.cut_split did it before the energy form: scores, then the detector on the float waveform."""
    sil = vad.ForwardSil(f32, is_final=True)
    seg = pkg.E2EVadModelHost()
    segs = seg(sil, f32[:400 + 160 * (sil.size - 1)], True, False, 800, 60000, 0.9)
    seg.close()
    frames = [(s * 16, min(e * 16, len(f32))) for s, e in segs]
    return frames, sorted(range(len(frames)), key=lambda i: (frames[i][1] - frames[i][0], i))


@pytest.fixture(scope="module")
def flow(pkg, weights_mod):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    vman, vblob = shape_vad_weights(*weights_mod.synth_vad_weights())
    vad = pkg.FsmnVadHip().InitVad((vman, vblob))
    s16 = make_file_s16(np.random.default_rng(61))
    f32 = s16.astype(np.float32) / np.float32(32768.0)
    want = frames_by_the_waveform_detector(pkg, vad, f32)
    yield {"vad": vad, "vman": vman, "vblob": vblob, "s16": s16, "f32": f32, "want": want}
    vad.close()


def test_cut_split_on_int16(pkg, flow):
    pipeline = importlib.import_module("asr_2pass_amd.pipeline")
    frames, index = flow["want"]
    assert len(frames) == 4                                    # four bursts
    for pcm in (flow["s16"], flow["f32"]):
        seg = pkg.E2EVadModelHost()
        got = pipeline.cut_split(pcm, flow["vad"], seg, 800, 60000, 0.9)
        seg.close()
        assert got == (frames, index)
    seg = pkg.E2EVadModelHost()
    assert pipeline.cut_split(flow["s16"][:399], flow["vad"], seg) == ([], [])
    seg.close()


def test_offline_handle_api_on_s16(pkg, weights_mod, flow, tmp_path):
    pipeline = importlib.import_module("asr_2pass_amd.pipeline")
    # a model with the timestamp head, as the other handle-API tests use: its text goes through PostProcess, which keeps no state.
    # (Without the head the text is Vocab::Vector2StringV2's, which by the reference's design depends on how the PREVIOUS call on the
    # object ended — the harness' first call and its later ones then differ in their blanks whatever the VAD does.)
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=300, timestamp=1)
    aman, ablob = weights_mod.synth_weights(cfg)
    mdir, vdir = tmp_path / "asr", tmp_path / "vad"
    mdir.mkdir(); vdir.mkdir()
    weights_mod.save(str(mdir / "model.pfhip"), aman, ablob)
    weights_mod.save(str(vdir / "vad.pfhip"), flow["vman"], flow["vblob"])
    with open(mdir / "tokens.json", "w") as f:
        json.dump([f"<{i}>" for i in range(300)], f)
    flow["s16"].tofile(tmp_path / "long.pcm")
    frames, index = flow["want"]
    asr = pkg.ParaformerHip().InitAsr((aman, ablob))
    seg = pkg.E2EVadModelHost()
    ids, got_frames = pipeline.infer_buffer(flow["f32"], asr, flow["vad"], seg, batch_size=4, vad_max_len=60000)
    seg.close(); asr.close()
    assert got_frames == frames
    exe = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "offline_infer")
    out = subprocess.run([exe, str(mdir), str(vdir), str(tmp_path / "long.pcm"), "4", "4", "2"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr                     # 4 threads re-run the file: 0 results differ (else exit 3)
    lines = out.stdout.splitlines()
    segs = [l for l in lines if l.startswith("seg ")]
    assert len(segs) == len(frames)
    for l, (s, e), want in zip(segs, frames, ids):
        head, _, tail = l.partition(":")
        assert [int(x) for x in head.split()[1:3]] == [s, e]
        assert [int(x) for x in tail.split()] == list(want)
    text = [l for l in lines if l.startswith("text ")][0][5:]
    assert text == "".join(" ".join(f"<{i}>" for i in seg_ids) for seg_ids in ids)
