"""GPU: time stamps from the CIF scan through the C++ adapter and the handle-API mirror (ParaformerHip::SetCifTimestamps,
FunOfflineSetCifStamps, FunTpassSetCifStamps: extensions, the reference stamps only through its timestamp head), run through the
`offline_infer` / `tpass_infer` harnesses as tests/test_gpu_nbest_adapter.py runs them.

The expected stamps are pfhip_cif_timestamps applied to the fire frames of a direct forward (forward_ids(want_fire_frames=True)) on
each VAD segment's samples, taken through the adapter's own text steps, restated in `expected_pairs`: the eos drop, the non-<sil>
spans, PostProcess's "%f" strings, the segment's start added in float, (int)(1000 * t).  batch = 1, so every segment is a forward of
its own in the harness as it is here: the same kernels, the same alphas, the same fire frames."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import ref_layout as RL
from test_gpu_pipeline import make_file, shape_vad_weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32 = np.float32
SPECIAL = ("<s>", "</s>", "<unk>")


def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")


def field(lines, name):
    return [l for l in lines if l.startswith(name + " ") or l == name][0][len(name) + 1:]


def segments(lines):
    segs = []
    for l in lines:
        if l.startswith("seg "):
            head, _, tail = l.partition(":")
            s, e = [int(x) for x in head.split()[1:3]]
            segs.append((s, e, [int(x) for x in tail.split()]))
    return segs


def expected_pairs(pkg, asr, tokens, pcm, segs, rate=16000):
    """[[begin_ms, end_ms], ...] as FunOfflineInferBuffer assembles them from ParaformerHip::Forward's "<text> | <stamps>" strings."""
    pairs, n_eos = [], 0
    for s, e, seg_ids in segs:
        r = asr.forward_ids([pcm[s:e]], want_fire_frames=True)
        assert list(r["ids"][0]) == seg_ids
        n = len(seg_ids)
        if n == 0:
            continue
        eos = tokens[seg_ids[-1]] == "</s>"
        n_eos += int(eos)
        n_chars = n - int(eos)
        if n_chars <= 0:
            continue
        spans = pkg.cif_timestamps(r["fire_frame"][0, :n], n_chars, int(r["n_frames"][0]), float(asr.lfr_frame_ms()))
        stamps = [(b, e2) for b, e2, sil in spans if not sil]
        assert len(stamps) == n_chars
        stamps += [(0.0, 0.0)] * (n - len(stamps))                       # the popped "</s>" is skipped before its stamp is read
        t0 = F32(s) / F32(rate)
        for i, tok in enumerate(seg_ids):
            if tokens[tok] in SPECIAL:                                     # PostProcess step 1: no character, no stamp
                continue
            b, e2 = (F32(float("%f" % v)) for v in stamps[i])              # std::to_string(float) and std::stof back
            pairs.append([int(F32(1000) * F32(b + t0)), int(F32(1000) * F32(e2 + t0))])
    return pairs, n_eos


def check_pairs(pairs, text, n_samples, rate=16000):
    assert len(pairs) == len(text) > 0                                     # one [b, e] per character of the (CJK) text
    assert all(b <= e for b, e in pairs)
    flat = [t for p in pairs for t in p]
    assert flat == sorted(flat)                                            # non-decreasing
    assert flat[0] >= 0 and flat[-1] <= n_samples * 1000 // rate           # within the audio


def run(args):
    out = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout[-3000:]
    return out.stdout.splitlines()


def test_plain_model_gets_stamps_from_fire_frames(pkg, weights_mod, tmp_path):
    """A plain model from a reference-layout directory: FunASRGetStamp is empty as ever with mode 0; with FunOfflineSetCifStamps(h, 1)
    it holds one [b, e] per character of the text, equal to the rule applied to the fire frames of direct forwards."""
    need_gpu()
    conv = importlib.import_module(pkg.__name__ + ".convert")
    rng = np.random.default_rng(13)
    pcm = make_file(rng)
    s16 = np.clip(np.round(pcm * 32768.0), -32768, 32767).astype("<i2")
    f32 = (s16.astype(np.float32) / 32768.0).astype(np.float32)            # what LoadPcmwav makes of the file
    vman, vblob = shape_vad_weights(*weights_mod.synth_vad_weights())
    V = 300
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=V)
    aman, ablob = weights_mod.synth_weights(cfg, seed=43)
    tokens = [chr(0x4E00 + i) for i in range(V - 3)] + list(SPECIAL)
    d = tmp_path / "asr"
    RL.write_asr_dir(str(d), conv, aman, ablob, cfg, vocab_tokens=tokens)
    RL.write_vad_dir(str(tmp_path / "vad"), conv, vman, vblob)
    s16.tofile(tmp_path / "long.pcm")
    asr = pkg.ParaformerHip().InitAsr(str(d / "model.onnx"), str(d / "am.mvn"), str(d / "config.yaml"), str(d / "tokens.json"))
    # the Python flow first (test_gpu_pipeline.py) says which id ends the first segment: that one is named "</s>", so that the eos drop
    # is on the path (a real model's tail slot emits it)
    pipeline = importlib.import_module("asr_2pass_amd.pipeline")
    vad = pkg.FsmnVadHip().InitVad((vman, vblob))
    seg = pkg.E2EVadModelHost()
    py_ids, _ = pipeline.infer_buffer(f32, asr, vad, seg, batch_size=1, vad_max_len=60000)
    vad.close(); seg.close()
    last = int(py_ids[0][-1])
    tokens = [chr(0x4E00 + i) for i in range(V)]
    tokens[last] = "</s>"
    with open(d / "tokens.json", "w") as f:
        json.dump(tokens, f)
    exe = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "offline_infer")
    lines = run([exe, str(d), str(tmp_path / "vad"), str(tmp_path / "long.pcm"), "1", "1", "1", "-", "16000", "0", "1"])
    assert field(lines, "stamp") == ""                                     # mode 0: a plain model has no stamps
    text = field(lines, "cif_text")
    assert text == field(lines, "text")
    segs = segments(lines)
    assert len(segs) == 5
    assert text == "".join(tokens[i] for _, _, ids in segs for i in ids if tokens[i] not in SPECIAL)
    got = json.loads(field(lines, "cif_stamp"))
    check_pairs(got, text, len(s16))
    want, n_eos = expected_pairs(pkg, asr, tokens, f32, segs)
    asr.close()
    assert n_eos >= 1
    print(f"{len(got)} stamps over {len(segs)} segments, {n_eos} segments end in </s>; first {got[:3]}, last {got[-2:]}")
    assert got == want


def test_timestamp_head_model_modes(pkg, weights_mod, tmp_path):
    """A model with the CifPredictorV3 head: mode 1 leaves the head's stamps as they are with mode 0; mode 2 skips the head and gives
    the CIF rule's."""
    need_gpu()
    rng = np.random.default_rng(11)
    pcm = make_file(rng)
    s16 = np.clip(np.round(pcm * 32768.0), -32768, 32767).astype("<i2")
    f32 = (s16.astype(np.float32) / 32768.0).astype(np.float32)
    vman, vblob = shape_vad_weights(*weights_mod.synth_vad_weights())
    V = 300
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=V, timestamp=1)
    aman, ablob = weights_mod.synth_weights(cfg)
    mdir, vdir = tmp_path / "asr", tmp_path / "vad"
    mdir.mkdir(); vdir.mkdir()
    weights_mod.save(str(mdir / "model.pfhip"), aman, ablob)
    weights_mod.save(str(vdir / "vad.pfhip"), vman, vblob)
    tokens = [chr(0x4E00 + i) for i in range(V)]
    with open(mdir / "tokens.json", "w") as f:
        json.dump(tokens, f)
    s16.tofile(tmp_path / "long.pcm")
    exe = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "offline_infer")
    base = [exe, str(mdir), str(vdir), str(tmp_path / "long.pcm"), "1", "1", "1", "-", "16000", "0"]
    one = run(base + ["1"])
    head = field(one, "stamp")
    assert head != "" and field(one, "cif_stamp") == head and field(one, "cif_text") == field(one, "text")
    two = run(base + ["2"])
    assert field(two, "stamp") == head and field(two, "cif_text") == field(two, "text")
    got = json.loads(field(two, "cif_stamp"))
    segs = segments(two)
    check_pairs(got, field(two, "text"), len(s16))
    asr = pkg.ParaformerHip().InitAsr((aman, ablob))
    want, _ = expected_pairs(pkg, asr, tokens, f32, segs)
    asr.close()
    assert got == want
    assert got != json.loads(head)                                         # they are not the head's stamps (20-ms grid, other rule)


def test_tpass_offline_pass_carries_stamps(pkg, weights_mod, tmp_path):
    """FunTpassSetCifStamps(h, 1): the second-pass results of the 2-pass flow carry stamps for a plain offline model; without it
    they carry none, and the texts are the same."""
    need_gpu()
    rng = np.random.default_rng(21)
    pcm = make_file(rng)[:16000 * 12]
    s16 = np.clip(np.round(pcm * 32768.0), -32768, 32767).astype("<i2")
    vman, vblob = shape_vad_weights(*weights_mod.synth_vad_weights())
    V = 300
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=V)
    aman, ablob = weights_mod.synth_weights(cfg, seed=31)
    oman, oblob = weights_mod.synth_weights(cfg, seed=77)
    dirs = {k: tmp_path / k for k in ("asr", "online", "vad")}
    for d in dirs.values():
        d.mkdir()
    weights_mod.save(str(dirs["asr"] / "model.pfhip"), aman, ablob)
    weights_mod.save(str(dirs["online"] / "model.pfhip"), oman, oblob)
    weights_mod.save(str(dirs["vad"] / "vad.pfhip"), vman, vblob)
    with open(dirs["asr"] / "tokens.json", "w") as f:
        json.dump([chr(0x4E00 + i) for i in range(V)], f)
    s16.tofile(tmp_path / "stream.pcm")
    exe = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "tpass_infer")
    base = [exe, str(dirs["asr"]), str(dirs["online"]), str(dirs["vad"]), str(tmp_path / "stream.pcm"), "9600", "2"]
    off = [l.split(" | ") for l in run(base) if l.startswith("call ")]
    on = [l.split(" | ") for l in run(base + ["-", "16000", "0", "1"]) if l.startswith("call ")]
    assert len(off) == len(on) > 5
    n_tpass = 0
    for a, b in zip(off, on):
        assert a[:3] == b[:3]                                              # call, online text, tpass text: unchanged
        assert a[3] == "stamp " or a[3] == "stamp"                         # a plain model: none
        text = b[2][len("tpass "):].strip()
        stamp = b[3][len("stamp"):].strip()
        if not text:
            assert stamp == ""
            continue
        n_tpass += 1
        pairs = json.loads(stamp)
        check_pairs(pairs, text, len(s16))
    assert n_tpass >= 2
