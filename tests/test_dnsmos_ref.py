"""CPU: the restatement of the DNSMOS networks (tests/dnsmos_ref.py) against known answers, its own fixtures and, where the reference
tree is present, the real files.

  * the clip loop's window arithmetic (dnsmos_local.py:59-77) on clips whose hop and skip counts were worked out by hand;
  * the polynomial maps against numpy's poly1d, as the reference calls them;
  * tests/golden/dnsmos_*.npz hold the files' initialisers bit for bit, and the hand-written networks equal a node-by-node walk of the
    files' own graphs (both skipped without the reference tree);
  * the float64 and float32 runs reproduce tests/golden/dnsmos_cases.npz.  float64 to 1e-9 (only the summation order of the BLAS
    differs between machines); float32 to 8 x the fixture's own |fp32 - fp64| and no less than 16 float32 ulp of the value: another
    machine's float32 convolution sums in another order, and that is the size of such a difference."""
import os

import numpy as np
import pytest

import dnsmos_ref as R

torch = pytest.importorskip("torch")
REF = "/root/reference/utils"
FILES = {"primary": os.path.join(REF, "DNSMOS/sig_bak_ovr.onnx"), "p808": os.path.join(REF, "DNSMOS/model_v8.onnx")}
need_ref = pytest.mark.skipif(not all(os.path.exists(p) for p in FILES.values()), reason="/root/reference not present")


@pytest.fixture(scope="module")
def weights():
    return {k: R.load_weights(k) for k in ("primary", "p808")}


@pytest.fixture(scope="module")
def cases():
    with np.load(os.path.join(R.GOLDEN, "dnsmos_cases.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("n_samples, extended, hops, scored", [
    (9 * 16000, 18 * 16000, 9, 7),                   # a 9-s clip doubles to 18 s
    (600 * 16000, 600 * 16000, 591, 570),            # ten minutes
    (144160, 144160, 1, 1),                          # exactly one window
    (175999, 175999, 1, 1),                          # one sample short of an 11th second
    (1, 1 << 18, 7, None),                           # one sample doubles 18 times
])
def test_clip_loop_known_answers(n_samples, extended, hops, scored):
    audio = R.extend_clip(np.zeros(n_samples, np.float32))
    assert len(audio) == extended
    num_hops, kept = R.clip_windows(len(audio))
    assert num_hops == hops
    if scored is not None:
        assert len(kept) == scored
    for b, e in kept:
        assert e - b == R.LEN_SAMPLES and b % R.FS == 0 and e <= len(audio)
    # every window that is not kept is one whose end the double arithmetic put one sample short
    short = [i for i in range(num_hops) if int((i + R.INPUT_LENGTH) * R.FS) - i * R.FS == R.LEN_SAMPLES - 1]
    assert len(short) == num_hops - len(kept)


def test_windows_skipped_in_the_nine_second_clip():
    """Which two: int((idx + 9.01) * 16000) falls one short of idx * 16000 + 144160 for idx = 4 and 8 (worked out in double here)."""
    _, kept = R.clip_windows(18 * 16000)
    skipped = sorted(set(range(9)) - {b // R.FS for b, _ in kept})
    assert skipped == [i for i in range(9) if int((i + 9.01) * 16000) < i * 16000 + 144160]
    assert len(skipped) == 2


@pytest.mark.parametrize("personalized", [False, True])
def test_polyfit_is_poly1d(personalized):
    sig, bak, ovr = 3.1, 2.2, 1.7
    c = R.POLY[personalized]
    want = (np.poly1d(c["sig"])(sig), np.poly1d(c["bak"])(bak), np.poly1d(c["ovr"])(ovr))
    assert R.polyfit(sig, bak, ovr, personalized) == pytest.approx(want, rel=0, abs=1e-15)
    assert len(c["sig"]) == (4 if personalized else 3)


def test_score_clip_means_and_counts():
    raw = np.array([[3.0, 1.0, 2.0, 3.0], [4.0, 2.0, 3.0, 4.0]])
    r = R.score_clip(raw, 9)
    assert (r["num_hops"], r["n_scored"]) == (9, 2)
    assert (r["p808"], r["sig_raw"], r["bak_raw"], r["ovr_raw"]) == (3.5, 1.5, 2.5, 3.5)
    assert r["sig"] == pytest.approx((R.polyfit(1, 2, 3, False)[0] + R.polyfit(2, 3, 4, False)[0]) / 2, abs=1e-15)
    p = R.score_clip(raw, 9, personalized=True)
    assert all(p[k] == r[k] for k in ("num_hops", "n_scored", "p808", "sig_raw", "bak_raw", "ovr_raw"))
    assert all(p[k] != r[k] for k in ("sig", "bak", "ovr"))


def test_mel_filters_are_slaney_triangles():
    w = R.mel_filters()
    assert w.shape == (120, 161) and (w >= 0).all()
    f = np.arange(161) * 16000.0 / 321
    # Slaney normalisation: every triangle has unit area over frequency.  The bins sample it every d = 49.8 Hz; the ten widest
    # triangles have half-widths h >= 170 Hz, and a Riemann sum of a triangle is off by at most (d / h)^2 / 3 < 0.03 of its area
    # (the narrow ones at the bottom, h = 67 Hz, are sampled once or twice and say nothing)
    area = (w * (16000.0 / 321)).sum(axis=1)
    assert np.abs(area[-10:] - 1.0).max() < 0.03
    # the peaks walk up the axis, the last triangle ends at 8 kHz: the last bin, 7975 Hz, still lies inside it
    peaks = f[w.argmax(axis=1)]
    assert (np.diff(peaks) >= 0).all() and peaks[0] < 100.0 and w[-1, -1] > 0


def test_melspec_of_silence_and_shape():
    m = R.melspec(np.zeros(R.MEL_SAMPLES))
    assert m.shape == (900, 120) and (m == 1.0).all()
    t = np.arange(R.MEL_SAMPLES) / 16000.0
    m = R.melspec(np.sin(2 * np.pi * 1000.0 * t))
    assert m.max() == 1.0 and m.min() == -1.0            # the reference itself, and the 80-dB floor: (-80 + 40) / 40


@need_ref
@pytest.mark.parametrize("kind", ["primary", "p808"])
def test_fixtures_hold_the_files_initialisers(pkg, weights, kind):
    from asr_2pass_amd import onnx_reader
    m = onnx_reader.read_model(FILES[kind])
    assert sorted(m.initializers) == sorted(weights[kind])
    for k, v in m.initializers.items():
        got = weights[kind][k]
        assert got.dtype == v.dtype and got.shape == v.shape and got.tobytes() == np.asarray(v).tobytes(), k


@need_ref
def test_restatement_equals_the_graph_walk(pkg, weights):
    from asr_2pass_amd import onnx_reader
    x = np.stack([R.case_window("tone_noise"), R.case_window("clipped_square")])
    with torch.no_grad():
        m = onnx_reader.read_model(FILES["primary"])
        env = R.walk_graph(m, {"input_1": x})
        got = R.primary_forward(weights["primary"], x)
        assert np.abs(env[m.outputs[0][0]].numpy() - got.numpy()).max() < 1e-12
        assert np.abs(env["mos_estimator_logpow/truediv:0"].numpy() - R.logpow(weights["primary"], x).numpy()).max() < 1e-12
        mel = np.stack([R.melspec(w[:R.MEL_SAMPLES]) for w in x])
        m = onnx_reader.read_model(FILES["p808"])
        env = R.walk_graph(m, {"input_1": mel})
        assert np.abs(env[m.outputs[0][0]].numpy() - R.p808_forward(weights["p808"], mel).numpy()).max() < 1e-12


def test_restatement_reproduces_the_cases(weights, cases):
    assert list(cases["names"]) == list(R.CASES)
    x = np.stack([R.case_window(c) for c in R.CASES])
    mel = np.stack([R.melspec(w[:R.MEL_SAMPLES]) for w in x])
    assert np.abs(mel.mean(axis=(1, 2)) - cases["mel_mean"]).max() < 1e-9
    with torch.no_grad():
        p64 = R.primary_forward(weights["primary"], x, torch.float64).numpy()
        p32 = R.primary_forward(weights["primary"], x, torch.float32).numpy()
        q64 = R.p808_forward(weights["p808"], mel, torch.float64).numpy()
        q32 = R.p808_forward(weights["p808"], mel.astype(np.float32), torch.float32).numpy()
    assert np.abs(p64 - cases["primary_f64"]).max() < 1e-9 and np.abs(q64 - cases["p808_f64"]).max() < 1e-9
    for got, f32, f64 in ((p32, cases["primary_f32"], cases["primary_f64"]), (q32, cases["p808_f32"], cases["p808_f64"])):
        bound = np.maximum(8 * np.abs(f32 - f64).max(), 16 * np.spacing(np.abs(f64).astype(np.float32)))
        err = np.abs(got.astype(np.float64) - f64)
        print("fp32 restatement: worst error", err.max(), "bound", bound.min())
        assert (err <= bound).all()
