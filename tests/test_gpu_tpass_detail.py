"""GPU: FunTpassSetNbest through the `tpass_infer` harness: per FunTpassInferBuffer call the confidences and fire times of the
streamed tokens (FunASRGetOnlineConfidence / FunASRGetOnlineFireMs) and the confidences of the second-pass text
(FunASRGetTokenConfidence), against the Python ParaformerOnlineHip.last_detail() run over the same frames.

Both runs feed one connection alone, so every forward has the same composition and the log-probabilities are the same bits; the
harness prints exp(logp) computed by the C library's expf, which is within one unit in the last place of the exact value, so a
confidence is compared with the float64 exp of the Python run's logp to one float32 spacing.  Fire times are integers: ==.
"""
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import audio_split as A
from test_gpu_pipeline import make_file, shape_vad_weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K = 3


def test_tpass_harness_detail(pkg, weights_mod, tmp_path):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    rng = np.random.default_rng(21)
    pcm = make_file(rng)[:16000 * 12]
    s16 = np.clip(np.round(pcm * 32768.0), -32768, 32767).astype("<i2")
    vman, vblob = shape_vad_weights(*weights_mod.synth_vad_weights())
    cfg = weights_mod.small_config(enc_layers=3, dec_layers=2, vocab=517)
    aman, ablob = weights_mod.synth_weights(cfg, seed=31)
    oman, oblob = weights_mod.synth_weights(cfg, seed=77)
    dirs = {k: tmp_path / k for k in ("asr", "online", "vad")}
    for d in dirs.values():
        d.mkdir()
    weights_mod.save(str(dirs["asr"] / "model.pfhip"), aman, ablob)
    weights_mod.save(str(dirs["online"] / "model.pfhip"), oman, oblob)
    weights_mod.save(str(dirs["vad"] / "vad.pfhip"), vman, vblob)
    s16.tofile(tmp_path / "stream.pcm")
    exe = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "tpass_infer")
    base = [exe, str(dirs["asr"]), str(dirs["online"]), str(dirs["vad"]), str(tmp_path / "stream.pcm"), "9600", "2"]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    flagged = subprocess.run(base + ["-", "16000", str(K)], capture_output=True, text=True, timeout=300)
    assert flagged.returncode == 0, flagged.stderr
    plain_lines = [l for l in plain.stdout.splitlines() if l.startswith("call ")]
    got = [l.split(" | ") for l in flagged.stdout.splitlines() if l.startswith("call ")]
    assert all(len(g) == 6 and g[4].startswith("online_detail") and g[5].startswith("tpass_conf") for g in got)
    # without the flag: the same lines without the two extra fields
    assert plain_lines == [" | ".join(g[:4]) for g in got]
    assert all(len(l.split(" | ")) == 4 for l in plain_lines)
    # ---- the same flow in Python, the streaming model with set_detail(K, True) -------------------------------------------
    vad = pkg.FsmnVadHip().InitVad((vman, vblob))
    asr = pkg.ParaformerHip().InitAsr((aman, ablob))
    asr_on_model = pkg.ParaformerHip().InitAsr((oman, oblob))
    vad_on = pkg.FsmnVadOnlineHip(vad, 800, 60000, 0.9)
    stream = pkg.ParaformerOnlineHip(asr_on_model)
    stream.set_detail(K, True)
    audio = A.TpassAudio()
    f32 = (s16.astype(np.float32) / 32768.0).astype(np.float32)
    n_online = n_tpass = 0
    for j, off in enumerate(range(0, len(f32), 9600)):
        last = off + 9600 >= len(f32)
        audio.LoadPcmwavOnline(f32[off:off + 9600])
        audio.Split(lambda w, fin: vad_on.Infer(w, fin), 9600, last, A.ASR_TWO_PASS)
        ids, logp0, fire_ms, online_txt = [], [], [], ""
        while True:
            fr = audio.FetchChunck()
            if fr is None:
                break
            piece = stream.Forward(fr["data"], input_finished=fr["is_final"])
            det = stream.last_detail()
            assert det["n"] == len(piece) and list(det["ids"][:, 0]) == piece
            ids += piece
            text = " ".join(str(i) for i in piece)
            online_txt += text + (" " if text and stream.last_path() == 2 else "")      # paraformer-online.cpp:585-587
            logp0 += [float(v) for v in det["logp"][:, 0]]
            fire_ms += [60 * int(f) for f in det["fire_frame"]]
            assert list(det["fire_ms"]) == [60 * int(f) for f in det["fire_frame"]]
        tpass_n = None
        while True:
            fr = audio.FetchTpass()
            if fr is None:
                break
            tpass_n = len(asr.forward_ids([fr["data"]])["ids"][0])
        if last:
            audio.ResetIndex()
        assert got[j][0] == f"call {j}"
        assert got[j][1] == "online " + online_txt, (j, got[j][1], online_txt)        # (no vocabulary: the ids are the text)
        entries = got[j][4].split()[1:]
        assert len(entries) == len(ids), (j, got[j][4], ids)                            # one entry per online id
        for e, lp, ms in zip(entries, logp0, fire_ms):
            conf, at = e.split("@")
            conf = np.float32(conf)
            assert int(at) == ms, (j, e, ms)
            assert abs(float(conf) - math.exp(lp)) <= float(np.spacing(conf)), (j, e, lp)
            assert 0.0 < conf <= 1.0
        tconf = [np.float32(x) for x in got[j][5].split()[1:]]
        if tpass_n:                                                                     # a segment closed in this call
            assert len(tconf) == tpass_n and all(0.0 < c <= 1.0 for c in tconf), (j, got[j][5])
            assert len(got[j][2].split()) - 1 == tpass_n
            n_tpass += 1
        else:
            assert tconf == []
        n_online += len(ids)
    assert len(got) == j + 1 and n_online > 0 and n_tpass >= 1
    for o in (vad_on, stream, vad, asr, asr_on_model):
        o.close()
