"""CPU: the end-point detector fed frame energies (pfhip_vadseg_feed_energy) returns exactly the segments it returns when fed
the waveform (pfhip_vadseg_feed), on the inputs of the tests/golden vadseg cases — offline, online and chunked online feeding.

The energies are computed here as the issue's reference does: one float32 accumulator per frame, samples in ascending order,
every product rounded to float32 before it is added (numpy float32 arithmetic neither fuses nor widens) — oracle/e2e_vad.py's
decibel track without the logarithm.  Since the golden segments came from the compiled reference, the energy path is pinned to
`funasr::E2EVadModel` as well."""
import glob
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = sorted(glob.glob(os.path.join(HERE, "golden", "vadseg_*.npz")))

spec = importlib.util.spec_from_file_location("make_vadseg_golden", os.path.join(HERE, "golden", "make_vadseg_golden.py"))
G = importlib.util.module_from_spec(spec)
spec.loader.exec_module(G)


def frame_energy_ref(w, flen=400, fshift=160):
    w = np.ascontiguousarray(w, dtype=np.float32)
    F = 0 if w.size < flen else 1 + (w.size - flen) // fshift
    s = np.zeros(F, np.float32)
    idx = np.arange(F) * fshift
    for i in range(flen):
        x = w[idx + i]
        s += x * x
    return s


def energy_feed(m):
    def feed(sil, wave, fin, online, max_end_sil, max_seg, thres):
        return m.feed_energy(sil, frame_energy_ref(wave), len(wave), fin, online, max_end_sil, max_seg, thres)
    return feed


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[7:-4] for p in GOLD])
def test_energy_feed_equals_waveform_feed(pkg, path):
    c = np.load(path)
    w = G.waveform(c["amp"], c["pattern"])
    mw, me = pkg.E2EVadModelHost(), pkg.E2EVadModelHost()
    want = G.run_plan(lambda *a: mw(*a), c["sil"], w, c["calls"], c["params"])
    got = G.run_plan(energy_feed(me), c["sil"], w, c["calls"], c["params"])
    mw.close()
    me.close()
    assert got.tolist() == want.tolist()
    assert got.tolist() == c["segs"].tolist()          # and both are the compiled reference's segments


def test_the_cases_cover_both_modes_and_chunked_feeding():
    modes = set()
    for p in GOLD:
        calls = np.load(p)["calls"]
        modes.add((bool(calls[:, 3].any()), len(calls) > 1))
    assert {(False, False), (False, True), (True, True)} <= modes       # offline whole, offline chunked, online chunked


def test_random_plans_energy_feed(pkg):
    """The 60 seeded random plans of the waveform test: random chunking, both modes, detector objects re-used across files."""
    c = np.load(os.path.join(HERE, "golden", "e2evad_random_plans.npz"))
    ends = np.cumsum(c["counts"])
    for trial, (sil, w, calls, params) in enumerate(G.random_plans()):
        want = c["segs"][ends[trial] - c["counts"][trial]:ends[trial]].tolist()
        m = pkg.E2EVadModelHost()
        assert G.run_plan(energy_feed(m), sil, w, calls, params).tolist() == want, trial
        m.close()


@pytest.mark.parametrize("n_samples,n_energy", [(16000, 97), (16000, 99), (399, 1), (400, 0), (560, 1), (0, 1)])
def test_wrong_energy_count_is_an_argument_error(pkg, n_samples, n_energy):
    m = pkg.E2EVadModelHost()
    right = 0 if n_samples < 400 else 1 + (n_samples - 400) // 160
    assert n_energy != right
    with pytest.raises(pkg.PfhipError, match="status 1"):
        m.feed_energy(np.full(min(n_energy, right), 0.5, np.float32), np.ones(n_energy, np.float32), n_samples, True, False)
    # the detector is untouched by the refused call: the right count is accepted
    m.feed_energy(np.full(right, 0.5, np.float32), np.ones(right, np.float32), n_samples, True, False)
    m.close()


def test_energy_count_follows_the_sample_rate(pkg):
    m = pkg.E2EVadModelHost()
    n = 8000                                                   # at 8 kHz: 200-sample windows, 80-sample shift
    right = 1 + (n - 200) // 80
    m.feed_energy(np.full(right, 0.9, np.float32), np.ones(right, np.float32), n, True, False, sample_rate=8000)
    with pytest.raises(pkg.PfhipError, match="status 1"):
        m.feed_energy(np.full(48, 0.9, np.float32), np.ones(48, np.float32), n, True, False, sample_rate=8000)
    m.close()
