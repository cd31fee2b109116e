"""GPU: the pfhip_mos_* family (csrc/mos.cpp) through DnsMosHip on the real weights: tests/golden/dnsmos_*.npz written out as .onnx
files by tests/dnsmos_onnx.py, turned into a "dnsmos" container by convert.convert_dnsmos and loaded with
pfhip_mos_create_from_memory; a second handle reads the same files with pfhip_mos_create_from_files (the C++ reader).

  * three windows — tone plus noise, all zeros, a clipped square — against tests/golden/dnsmos_cases.npz: each of the four outputs
    within max(8 x the fixture's worst |fp32 - fp64|, 16 float32 ulp at the output's magnitude) of the float64 value;
  * the clip-level result of a 9-s clip (9 hops, 7 scored) equals the restated loop (tests/dnsmos_ref.py) on the same per-window
    values: counts exact, means to 1e-6;
  * bit for bit: 16-bit samples against the float32 call, a clip alone against the same clip in a batch of three, 2-window slabs
    against one slab, personalised against plain everywhere but sig / bak / ovr, and the handle made from the files against the one
    made from memory;
  * the clip loop inside the library on the issue's other known answers: ten minutes (591 hops, 570 scored), 175999 samples (1 hop),
    one sample (doubled 18 times: 7 hops), an empty clip refused.

Measured on an MI355X: worst |error| of the twelve outputs against float64 1.116e-06, where the fixture's own worst |fp32 - fp64| is
1.029e-06 and the smallest bound 8.235e-06."""
import os

import numpy as np
import pytest

import dnsmos_onnx as O
import dnsmos_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("dnsmos")
    p, q = d / "sig_bak_ovr.onnx", d / "model_v8.onnx"
    p.write_bytes(O.primary_onnx(R.load_weights("primary")))
    q.write_bytes(O.p808_onnx(R.load_weights("p808")))
    return str(p), str(q)


@pytest.fixture(scope="module")
def mos(pkg, files):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    import importlib
    conv = importlib.import_module("asr_2pass_amd.convert")
    m = pkg.DnsMosHip().InitMos(conv.convert_dnsmos(files[0], files[1]), device=0)          # pfhip_mos_create_from_memory
    yield m
    m.close()


@pytest.fixture(scope="module")
def cases():
    with np.load(os.path.join(R.GOLDEN, "dnsmos_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def nine_second_clip():
    rng = np.random.default_rng(99)
    t = np.arange(9 * 16000) / 16000.0
    x = 9000.0 * (0.5 * np.sin(2 * np.pi * 330.0 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3.0 * t)) + 0.3 * rng.standard_normal(t.size))
    return (np.clip(np.round(x), -32768, 32767) / 32768.0).astype(np.float32)


@pytest.fixture(scope="module")
def nine(mos):
    clip = nine_second_clip()
    hops, scored, raw = mos.score_windows([clip])
    return clip, hops, scored, raw


def test_windows_against_the_cases(mos, cases):
    wins = [R.case_window(c) for c in R.CASES]
    hops, scored, raw = mos.score_windows(wins)
    assert hops == [1, 1, 1] and scored == [1, 1, 1] and raw.shape == (3, 4)
    f64 = np.concatenate([cases["p808_f64"], cases["primary_f64"]], axis=1)
    f32 = np.concatenate([cases["p808_f32"], cases["primary_f32"]], axis=1).astype(np.float64)
    worst32 = np.abs(f32 - f64).max()
    bound = np.maximum(8 * worst32, 16 * np.spacing(np.abs(f64).astype(np.float32)).astype(np.float64))
    err = np.abs(raw.astype(np.float64) - f64)
    print(f"windows: worst error {err.max():.3e}, fixture's worst |fp32 - fp64| {worst32:.3e}, smallest bound {bound.min():.3e}")
    assert (err <= bound).all()


def test_nine_second_clip_equals_the_restated_loop(mos, nine):
    clip, hops, scored, raw = nine
    assert hops == [9] and scored == [7] and raw.shape == (7, 4)
    n_hops, kept = R.clip_windows(len(R.extend_clip(clip)))
    assert (n_hops, len(kept)) == (9, 7)
    for personalized in (False, True):
        got = mos.score([clip], personalized)[0]
        want = R.score_clip(raw, n_hops, personalized)
        assert (got["num_hops"], got["n_scored"]) == (want["num_hops"], want["n_scored"]) == (9, 7)
        for k in ("p808", "sig_raw", "bak_raw", "ovr_raw", "sig", "bak", "ovr"):
            assert abs(got[k] - want[k]) <= 1e-6, k
    # the windows are the doubled clip's: window 1 of the clip is the same samples as a clip cut there
    doubled = R.extend_clip(clip)
    _, _, alone = mos.score_windows([doubled[kept[1][0]:kept[1][1]]])
    assert alone.tobytes() == raw[1:2].tobytes()


def test_s16_bits_equal_f32_bits(mos, nine):
    clip, _, _, raw = nine
    s16 = np.round(clip * 32768.0).astype(np.int16)
    assert np.array_equal(s16.astype(np.float32) / np.float32(32768.0), clip)
    _, _, got = mos.score_windows([s16])
    assert got.tobytes() == raw.tobytes()


def test_alone_equals_in_a_batch_of_three(mos, nine):
    clip, _, _, raw = nine
    others = [R.case_window("clipped_square"), R.case_window("tone_noise")[:20000]]
    hops, scored, got = mos.score_windows([others[0], clip, others[1]])
    assert hops[1] == 9 and scored[1] == 7
    assert got[scored[0]:scored[0] + 7].tobytes() == raw.tobytes()


def test_two_window_slabs_equal_one_slab(mos, nine):
    clip, _, _, raw = nine
    # two ping-pong buffers of the largest activation tensor (900 x 161 x 128 floats) for two windows: slabs of 2, 2, 2, 1
    mos.set_workspace(2 * 2 * 900 * 161 * 128 * 4)
    try:
        _, _, got = mos.score_windows([clip])
        mos.set_workspace(1)                                     # below one window: one window at a time still runs
        _, _, one = mos.score_windows([clip])
    finally:
        mos.set_workspace(2 << 30)
    assert got.tobytes() == raw.tobytes() and one.tobytes() == raw.tobytes()


def test_personalised_differs_only_in_the_fitted_fields(mos, nine):
    clip = nine[0]
    a, b = mos.score([clip], False)[0], mos.score([clip], True)[0]
    for k in ("num_hops", "n_scored", "p808", "sig_raw", "bak_raw", "ovr_raw"):
        assert a[k] == b[k], k
    for k in ("sig", "bak", "ovr"):
        assert a[k] != b[k], k


def test_second_handle_gives_the_same_bits(pkg, files, nine):
    clip, _, _, raw = nine
    m = pkg.DnsMosHip().InitMos(files[0], files[1])          # pfhip_mos_create_from_files: the C++ reader
    try:
        _, _, got = m.score_windows([clip])
    finally:
        m.close()
    assert got.tobytes() == raw.tobytes()
    m = pkg.DnsMosHip().InitMos(files[0])          # without the P.808 net: its column is NaN, the rest the same bits
    try:
        _, _, got = m.score_windows([clip])
    finally:
        m.close()
    assert np.isnan(got[:, 0]).all() and got[:, 1:].tobytes() == np.ascontiguousarray(raw[:, 1:]).tobytes()


def test_clip_loop_in_the_library(mos, pkg):
    rng = np.random.default_rng(3)
    ten = (rng.standard_normal(600 * 16000) * 0.05).astype(np.float32)
    hops, scored, raw = mos.score_windows([ten, ten[:175999], ten[:1], ten[:144160]])
    assert hops == [591, 1, 7, 1] and scored[:2] == [570, 1] and scored[3] == 1
    assert scored[2] == len(R.clip_windows(1 << 18)[1]) and raw.shape == (sum(scored), 4) and np.isfinite(raw).all()
    # window 0 of the ten-minute clip is the 144160-sample clip's only window
    assert raw[0].tobytes() == raw[-1].tobytes()
    with pytest.raises(pkg.PfhipError):
        mos.score_windows([ten[:0]])
    with pytest.raises(pkg.PfhipError):
        pkg.DnsMosHip().InitMos(({"config": {"kind": "punc"}, "tensors": {}, "total_bytes": 0}, np.zeros(4, np.float32)))
