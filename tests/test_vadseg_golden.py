"""CPU: the end-point detector pinned to the REFERENCE compiled here (SURVEY §8 rows c, f1).

tests/golden/vadseg_*.npz were produced by `funasr::E2EVadModel` itself (onnxruntime/src/e2e-vad.h, compiled in place into
oracle/_ref/libe2evad_ref.so; generator tests/golden/make_vadseg_golden.py).  Both the oracle restatement
(oracle/e2e_vad.py) and the product's C++ detector (csrc/host/vad_segmenter.cpp through pfhip_vadseg_feed) must reproduce
every call's segments bit-exactly (integers).  The reference's segments for 60 seeded random plans are stored as well
(tests/golden/e2evad_random_plans.npz); where the compiled reference is present it is also driven directly on those plans."""
import glob
import importlib.util
import os

import numpy as np
import pytest

from oracle import e2e_vad as E

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = sorted(glob.glob(os.path.join(HERE, "golden", "vadseg_*.npz")))
REF_SO = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libe2evad_ref.so")

spec = importlib.util.spec_from_file_location("make_vadseg_golden", os.path.join(HERE, "golden", "make_vadseg_golden.py"))
G = importlib.util.module_from_spec(spec)
spec.loader.exec_module(G)


def test_fixture_set_is_complete():
    names = {os.path.basename(p)[7:-4] for p in GOLD}
    assert {"all_silence", "single_burst", "max_segment_split", "online_1s_feeds", "low_energy", "reuse_offline", "reuse_online",
            "online_irregular", "speech_to_eof_offline", "speech_to_eof_online", "online_empty_final", "offline_chunked"} <= names


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[7:-4] for p in GOLD])
def test_oracle_reproduces_reference_segments(path):
    c = np.load(path)
    m = E.E2EVadModel()
    got = G.run_plan(lambda *a: m(*a), c["sil"], G.waveform(c["amp"], c["pattern"]), c["calls"], c["params"])
    assert got.tolist() == c["segs"].tolist()


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[7:-4] for p in GOLD])
def test_product_reproduces_reference_segments(pkg, path):
    c = np.load(path)
    m = pkg.E2EVadModelHost()
    got = G.run_plan(lambda *a: m(*a), c["sil"], G.waveform(c["amp"], c["pattern"]), c["calls"], c["params"])
    m.close()
    assert got.tolist() == c["segs"].tolist()


def test_known_consequences_of_the_goldens():
    """Sanity on the fixtures themselves (hand-derivable from e2e-vad.h's constants): forced splits are exactly
    max_single_segment_time + one frame apart (:672-690: `cur_frm_idx - confirmed_start_frame + 1 > 600` fires at the 601st
    frame); online open/close markers alternate; an empty final call closes nothing."""
    c = np.load(os.path.join(HERE, "golden", "vadseg_max_segment_split.npz"))
    s = c["segs"]
    assert [int(e - b) for _, b, e in s[:3]] == [6010, 6010, 6010] and all(s[i][2] == s[i + 1][1] for i in range(3))
    c = np.load(os.path.join(HERE, "golden", "vadseg_online_1s_feeds.npz"))
    marks = [(int(b) >= 0, int(e) >= 0) for _, b, e in c["segs"]]
    assert marks == [(True, False), (False, True)] * 3
    c = np.load(os.path.join(HERE, "golden", "vadseg_online_empty_final.npz"))
    assert c["segs"].tolist() == [[1, 280, -1]]


def test_random_plans_against_the_compiled_reference(pkg):
    """60 seeded random plans (G.random_plans) against the segments the compiled reference returned for them
    (tests/golden/e2evad_random_plans.npz); where the compiled reference is present it must still return exactly those."""
    c = np.load(os.path.join(HERE, "golden", "e2evad_random_plans.npz"))
    ends = np.cumsum(c["counts"])
    plans = list(G.random_plans())
    assert len(plans) == len(ends) and ends[-1] == len(c["segs"])
    lib = G.load_ref() if os.path.exists(REF_SO) else None
    for trial, (sil, w, calls, params) in enumerate(plans):
        want = c["segs"][ends[trial] - c["counts"][trial]:ends[trial]].tolist()
        if lib is not None:
            assert G.ref_plan(lib, sil, w, calls, params).tolist() == want, ("reference", trial)
        mo, mp = E.E2EVadModel(), pkg.E2EVadModelHost()
        assert G.run_plan(lambda *a: mo(*a), sil, w, calls, params).tolist() == want, ("oracle", trial)
        assert G.run_plan(lambda *a: mp(*a), sil, w, calls, params).tolist() == want, ("product", trial)
        mp.close()
