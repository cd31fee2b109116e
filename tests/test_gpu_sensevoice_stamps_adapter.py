"""GPU: token time stamps for SenseVoiceSmall through the C++ adapter (SenseVoiceSmallHip::SetCtcTimestamps, FunOfflineSetCtcStamps)
and the `svs_infer` harness.  Switched off, the harness prints what it printed before; switched on, every text token (the kept ids
behind the four tags) gets one [begin_ms, end_ms] pair: the spans of pfhip_svs_align — compared with the Python mirror's align() on
the same samples — times pfhip_lfr_frame_ms, speech row 0 at 0 ms.  FunASRGetStamp carries them in its usual "[[b,e],...]" form and
stays empty when a decoder is attached."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_sensevoice_adapter as A

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

setup = A.setup
FRAME_MS = 60


def harness(s, args):
    env = dict(os.environ, PFHIP_WARMUP_SECONDS="0")
    r = subprocess.run([s["exe"]] + [str(a) for a in args], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def files(s):
    return [s["dir"] / f"utt{i}.pcm" for i in range(3)]


def ints(out, key):
    (line,) = [ln for ln in out.splitlines() if ln.startswith(key + " :")]
    return [int(x) for x in line.partition(" :")[2].split()]


def test_off_prints_what_it_printed_and_on_adds_one_pair_per_text_token(setup):
    s = setup
    args = [s["container"], "-", "en", "1"] + files(s)
    off = harness(s, args)
    on = harness(s, ["--ctc-stamps"] + args)
    assert " spans :" not in off and " stamps :" not in off
    kept = [ln for ln in on.splitlines(keepends=True) if " spans :" not in ln and " stamps :" not in ln]
    assert "".join(kept) == off                                      # nothing else moved
    ref = s["model"].forward(s["utts"], lang="en", itn=True)
    al = s["model"].align([ids[4:] for ids in ref["ids"]])
    n_pairs = 0
    for b in range(3):
        ids = ints(on, f"utt {b} ids")
        spans, stamps = ints(on, f"utt {b} spans"), ints(on, f"utt {b} stamps")
        text_tokens = max(len(ids) - 4, 0)
        assert len(spans) == len(stamps) == 2 * text_tokens          # one pair per text token
        assert spans[0::2] == al["begin"][b].tolist() and spans[1::2] == al["end"][b].tolist()
        assert stamps == [(r - 4) * FRAME_MS for r in spans]
        assert all(x < y for x, y in zip(stamps[0::2], stamps[1::2])) and all(e <= b2 for e, b2 in zip(stamps[1::2], stamps[2::2]))
        rows = int(ref["frame_len"][b])
        assert all(0 <= x <= (rows - 4) * FRAME_MS for x in stamps)
        n_pairs += text_tokens
    assert n_pairs > 10 and ints(on, "utt 1 stamps") == []            # utterance 1 has no frame


def test_funasr_get_stamp(setup):
    s = setup
    args = ["--handle-api", s["dir"], "en", "1", s["dir"] / "utt2.pcm"]
    off = harness(s, args)
    on = harness(s, ["--ctc-stamps"] + args)
    assert "handle stamp" not in off
    assert "".join(ln for ln in on.splitlines(keepends=True) if not ln.startswith("handle stamp [")) == off
    (stamp,) = [ln for ln in on.splitlines() if ln.startswith("handle stamp [")]
    ref = s["model"].forward([s["utts"][2]], lang="en", itn=True)
    al = s["model"].align([ref["ids"][0][4:]])
    pairs = [[(int(b) - 4) * FRAME_MS, (int(e) - 4) * FRAME_MS] for b, e in zip(al["begin"][0], al["end"][0])]
    assert len(pairs) == len(ref["ids"][0]) - 4 > 0
    want = "[" + ",".join(f"[{b},{e}]" for b, e in pairs) + "]"      # without a VAD the buffer is one segment at offset 0
    assert stamp == f"handle stamp [{want}]"
    with_dec = harness(s, ["--ctc-stamps", "--with-decoder"] + args)
    assert "handle stamp []" in with_dec.splitlines()


def test_no_stamps_with_a_decoder_handle(setup):
    s = setup
    out = harness(s, ["--ctc-stamps", "--decoder", s["container"]] + files(s))
    assert [ln for ln in out.splitlines() if " stamps " in ln] == [f"utt {i} stamps 0" for i in range(3)] * 2
