"""Resampling plan (host, no GPU): the NumPy restatement (tests/resample_ref.py), pfhip_resample_len and pfhip_op_resample_table
against recordings of the reference's own resampler.

Fixtures tests/golden/resample_<fs>.npz: outputs, first_index and weight rows of the reference's own LinearResample
(onnxruntime/src/resample.cpp, compiled with -fPIC -g as its CMakeLists sets; -O2 gives the same bits) run as
Audio::WavResample runs it (cutoff 0.99*0.5*min(fs_in,16000), 6 zeros, flush=true) on seeded int16 inputs / 32768.
Each file repeats this provenance string.
"""
import glob
import os

import numpy as np
import pytest

import resample_ref as R

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "resample_*.npz")))


def test_goldens_present():
    rates = sorted(int(np.load(p)["fs_in"]) for p in GOLDEN)
    assert rates == [8000, 11025, 12345, 22050, 32000, 44100, 48000]
    for p in GOLDEN:
        assert "LinearResample" in str(np.load(p)["provenance"])


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_restatement_bitwise_equals_reference(path):
    d = np.load(path)
    fs = int(d["fs_in"])
    P, first, nt, w = R.plan(fs, 16000)
    np.testing.assert_array_equal(first, d["first_index"])
    np.testing.assert_array_equal(nt, d["ntaps"])
    assert w.tobytes() == d["weights"].tobytes()
    for i, n in enumerate(d["lengths"]):
        x = d[f"in_{i}"].astype(np.float32) / np.float32(32768.0)
        y = R.resample(x, fs)
        assert y.shape[0] == R.out_len(fs, 16000, int(n))
        assert y.tobytes() == d[f"out_{i}"].tobytes(), (fs, int(n))


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_library_plan_equals_reference(pkg, path):
    d = np.load(path)
    fs = int(d["fs_in"])
    P, first, nt, w = pkg.resample_table(fs, 16000)
    np.testing.assert_array_equal(first, d["first_index"])
    np.testing.assert_array_equal(nt, d["ntaps"])
    assert w.tobytes() == d["weights"].tobytes()
    assert P == fs // np.gcd(fs, 16000)
    for i, n in enumerate(d["lengths"]):
        assert pkg.resample_len(fs, int(n)) == d[f"out_{i}"].shape[0]


@pytest.mark.parametrize("fs_in,fs_out", [(7999, 16000), (16001, 16000), (96000, 16000), (24000, 16000), (1000, 16000),
                                          (192000, 16000), (16000, 8000), (16000, 44100), (191999, 1000)])
def test_library_plan_equals_restatement(pkg, fs_in, fs_out):
    P, first, nt, w = pkg.resample_table(fs_in, fs_out)
    P2, first2, nt2, w2 = R.plan(fs_in, fs_out)
    assert P == P2
    np.testing.assert_array_equal(first, first2)
    np.testing.assert_array_equal(nt, nt2)
    assert w.tobytes() == w2.tobytes()


def test_lengths_many_pairs(pkg):
    rng = np.random.default_rng(7)
    rates = [1000, 7999, 8000, 11025, 12000, 16000, 16001, 22050, 24000, 32000, 44100, 48000, 96000, 192000]
    for fs_in in rates:
        for fs_out in (16000, 8000, 48000):
            for n in [0, 1, 2, 3, 5, 12, 13, 159, 160, 161, 1023, 1024, 16000, 480000] + list(rng.integers(0, 2_000_000, 8)):
                assert pkg.resample_len(fs_in, int(n), fs_out) == R.out_len(fs_in, fs_out, int(n)), (fs_in, fs_out, n)
    assert pkg.resample_len(16000, 12345) == 12345        # identity
    assert pkg.resample_len(48000, 48000 * 30) == 16000 * 30
    assert pkg.resample_len(8000, 8000 * 30) == 16000 * 30


@pytest.mark.parametrize("fs_in,fs_out", [(999, 16000), (192001, 16000), (0, 16000), (-8000, 16000), (16000, 200000),
                                          (191999, 16001), (160001, 16000)])
def test_unsupported_pairs_refused(pkg, fs_in, fs_out):
    # 191999 * 16001 overflows int32 (lcm), as does 160001 * 16000 = 2.56e9 (gcd 1)
    assert pkg.resample_len(fs_in, 1000, fs_out) == -1
    assert not R.supported(fs_in, fs_out)
    with pytest.raises(pkg.PfhipError):
        pkg.resample_table(fs_in, fs_out)


def test_lcm_bound_is_int32():
    assert R.supported(16001, 16000)                      # lcm 256 016 000
    assert not R.supported(160001, 16000)
    assert R.supported(134000, 16000) and R.supported(191998, 16000)
