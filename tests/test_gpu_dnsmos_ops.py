"""GPU: the kernels of the DNSMOS speech-quality networks through their operator entries (csrc/conv3x3.hip, csrc/dnsmos.hip) against
float64 restatements (tests/dnsmos_ref.py).

The bound of every comparison is the project's rule for fp32-grade arithmetic: 4 x the largest error that the SAME computation in
float32 on the CPU (torch / numpy) commits against float64 on the same case — the kernels claim to be as close to fp64 as an fp32
chain, and that is what an fp32 chain gives.  Error and bound are printed before every assert.

Measured on an MI355X (error / bound): see each test's docstring."""
import os

import numpy as np
import pytest

import dnsmos_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional
CANARY = 64
SENTINEL = -7777.25


def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")


@pytest.fixture(scope="module")
def ops(pkg):
    need_gpu()
    import importlib
    return importlib.import_module("asr_2pass_amd.ops")


@pytest.fixture(scope="module")
def weights():
    return {k: R.load_weights(k) for k in ("primary", "p808")}


@pytest.fixture(scope="module")
def cases():
    with np.load(os.path.join(R.GOLDEN, "dnsmos_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def out_with_canary(n):
    buf = torch.full((n + CANARY,), SENTINEL, dtype=torch.float32, device="cuda")
    return buf


def check_canary(buf, n):
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENTINEL).all()), "the canary behind the output was written"
    assert not bool((buf[:n] == SENTINEL).any()), "an output value was not written"


def report(what, got, f64, f32):
    err = float(np.abs(np.asarray(got, np.float64) - f64).max())
    bound = 4.0 * float(np.abs(np.asarray(f32, np.float64) - f64).max())
    print(f"{what}: error {err:.3e}  bound {bound:.3e}  ratio {err / bound if bound else float('inf'):.3f}")
    return err, bound


def conv_ref(x_nhwc, w, b, pool, dtype):
    h = torch.as_tensor(x_nhwc).to(dtype).permute(0, 3, 1, 2)
    y = F.relu(F.conv2d(h, torch.as_tensor(w).to(dtype), torch.as_tensor(b).to(dtype), stride=1, padding=1))
    if pool:
        y = F.max_pool2d(y, 2, 2)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


# N, H, W, Cin, Cout, pool
CONV_CASES = [(2, 5, 7, 1, 32, False), (1, 3, 3, 32, 32, True), (1, 9, 161, 64, 32, True), (3, 33, 19, 128, 64, False),
              (1, 225, 40, 32, 32, True), (1, 1, 1, 32, 64, False)]


@pytest.mark.parametrize("N, H, W, Cin, Cout, pool", CONV_CASES)
def test_conv3x3_relu_against_fp64(ops, N, H, W, Cin, Cout, pool):
    """Conv + bias + ReLU (+ 2x2 floor pool) against float64.  Activations as the networks have them (a log spectrum in [-12, 4] for
    Cin = 1, ReLU outputs up to ~5 otherwise), zero-mean weights and a small negative bias: about half of the pre-activations are
    negative, so a ReLU taken after the pool's maximum of the accumulators or before it, a pool over the wrong four pixels or a
    dropped last odd row all show.

    Measured error / bound (= 4 x the float32 torch convolution's own error), in case order: 2.135e-06 / 8.541e-06,
    9.563e-07 / 2.038e-06, 2.807e-06 / 1.524e-05, 6.005e-06 / 2.528e-05, 2.656e-06 / 1.519e-05, 3.455e-07 / 4.575e-07."""
    rng = np.random.default_rng(1000 * H + 10 * W + Cin)
    if Cin == 1:
        x = rng.uniform(-12.0, 4.0, (N, H, W, 1)).astype(np.float32)
    else:
        x = np.maximum(0.0, rng.normal(0.5, 1.5, (N, H, W, Cin))).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9.0 * Cin)).astype(np.float32)
    b = (rng.standard_normal(Cout) * 0.2 - 0.1).astype(np.float32)
    with torch.no_grad():
        f64, f32 = conv_ref(x, w, b, pool, torch.float64), conv_ref(x, w, b, pool, torch.float32)
        unpooled = conv_ref(x, w, b, False, torch.float64)
    assert (unpooled == 0).mean() > 0.2, "the case must have negative pre-activations"
    n = f64.size
    buf = out_with_canary(n)
    xd = dev(x.reshape(N, H, W) if Cin == 1 else x)
    ops.conv3x3_relu(xd, dev(w), dev(b), pool=pool, out=buf)
    check_canary(buf, n)
    got = buf[:n].cpu().numpy().reshape(f64.shape)
    err, bound = report(f"conv3x3 {N}x{H}x{W} {Cin}->{Cout} pool={pool}", got, f64, f32)
    assert err <= bound


def test_conv3x3_refuses_what_it_does_not_take(ops, pkg):
    x = torch.zeros((1, 4, 4, 48), device="cuda")
    with pytest.raises(pkg.PfhipError):
        ops.conv3x3_relu(x, torch.zeros((32, 48, 3, 3), device="cuda"), torch.zeros(32, device="cuda"))       # Cin % 32
    x = torch.zeros((1, 4, 4, 96), device="cuda")
    with pytest.raises(pkg.PfhipError):
        ops.conv3x3_relu(x, torch.zeros((32, 96, 3, 3), device="cuda"), torch.zeros(32, device="cuda"))       # not whole 64-channel stages
    x = torch.zeros((1, 4, 4, 32), device="cuda")
    with pytest.raises(pkg.PfhipError):
        ops.conv3x3_relu(x, torch.zeros((48, 32, 3, 3), device="cuda"), torch.zeros(48, device="cuda"))       # Cout
    w = torch.zeros((32, 32, 3, 3), device="cuda")
    w[3, 5, 1, 1] = float("inf")
    with pytest.raises(pkg.PfhipError):
        ops.conv3x3_relu(x, w, torch.zeros(32, device="cuda"))                                               # a weight outside the fp16 planes


# ---- the primary net's front end -----------------------------------------------------------------------------------------------------
def logpow_ref(W, wins, n_frames, dtype):
    """R.logpow on windows of 160 (n_frames + 1) samples."""
    x = torch.as_tensor(np.stack(wins)).to(dtype)
    fr = torch.cat([x[:, :160 * n_frames].reshape(-1, n_frames, 160), x[:, 160:].reshape(-1, n_frames, 160)], dim=2)
    wr = torch.as_tensor(W["time2freq/stft-real/kernel:0"][:, :, 0]).to(dtype)
    wi = torch.as_tensor(W["time2freq/stft-imag/kernel:0"][:, :, 0]).to(dtype)
    re, im = fr @ wr.T, fr @ wi.T
    p = torch.maximum(torch.as_tensor(1e-12).to(dtype), torch.sqrt(re * re + im * im) ** 2)
    return (torch.log(p) / torch.as_tensor(np.float32(2.3025851)).to(dtype)).numpy()


def run_logpow(ops, W, pcm, offs, n_frames):
    n = len(offs) * n_frames * 161
    buf = out_with_canary(n)
    ops.dnsmos_logpow(dev(pcm), offs, dev(W["time2freq/stft-real/kernel:0"]), dev(W["time2freq/stft-imag/kernel:0"]), n_frames=n_frames,
                      floor=float(W["mos_estimator_logpow/Maximum/x:0"]), power=float(W["mos_estimator_logpow/pow/y:0"]),
                      denom=float(W["mos_estimator_logpow/truediv/y:0"]), out=buf)
    check_canary(buf, n)
    return buf[:n].cpu().numpy().reshape(len(offs), n_frames, 161)


def test_logpow_zero_window_is_the_floor(ops, weights):
    """All-zero samples: every bin of every frame holds the floor's value, log(1e-12) / 2.3025851, the same bits everywhere.  The value
    is one float32 logarithm (1 ulp on the device) and one correctly rounded division: within 2 ulp of the float64 value.  "Exactly
    the floor value" is read as that on purpose: the bits of the device's logf(1e-12f) are not the host library's to the last ulp, so
    the test pins equality across all bins bit for bit and the value itself to the 2 ulp that one logf and one division can cost."""
    W = weights["primary"]
    got = run_logpow(ops, W, np.zeros(R.LEN_SAMPLES, np.float32), [0], R.N_FRAMES)
    assert (got == got.flat[0]).all()
    want = np.log(np.float64(np.float32(1e-12))) / np.float64(np.float32(2.3025851))
    assert abs(float(got.flat[0]) - want) <= 2 * np.spacing(np.float32(abs(want)))


def test_logpow_against_fp64(ops, weights):
    """Tone plus noise and the full-scale clipped square, whole windows of 900 frames, plus three overlapping 13-frame windows at odd
    sample offsets (13 is no multiple of the 8 frames a workgroup takes); against float64 on the same float32 samples.

    Measured error / bound: tone plus noise 1.354e-04 / 4.417e-03 (bins where the spectrum nearly cancels: the logarithm magnifies
    both errors), clipped square 1.008e-05 / 5.410e-05, 13-frame windows 4.718e-06 / 3.397e-05."""
    W = weights["primary"]
    for name in ("tone_noise", "clipped_square"):
        x = R.case_window(name)
        got = run_logpow(ops, W, x, [0], R.N_FRAMES)
        with torch.no_grad():
            f64, f32 = R.logpow(W, x[None], torch.float64).numpy(), R.logpow(W, x[None], torch.float32).numpy()
        err, bound = report(f"logpow {name}", got, f64, f32)
        assert err <= bound
    x = R.case_window("tone_noise")[:40000]
    offs, nf = [1, 16001, 40000 - 160 * 14], 13
    wins = [x[o:o + 160 * (nf + 1)] for o in offs]
    got = run_logpow(ops, W, x, offs, nf)
    with torch.no_grad():
        f64, f32 = logpow_ref(W, wins, nf, torch.float64), logpow_ref(W, wins, nf, torch.float32)
    err, bound = report("logpow 13-frame windows", got, f64, f32)
    assert err <= bound


def test_logpow_s16_bits_equal_f32_bits(ops, weights):
    W = weights["primary"]
    rng = np.random.default_rng(5)
    s = rng.integers(-32768, 32768, 50001).astype(np.int16)
    s[:100] = [-32768, 32767] * 50
    offs, nf = [0, 1, 50001 - 160 * 21], 20
    a = run_logpow(ops, W, s, offs, nf)
    b = run_logpow(ops, W, s.astype(np.float32) / np.float32(32768.0), offs, nf)
    assert a.tobytes() == b.tobytes()


def test_logpow_refuses_a_window_outside_the_samples(ops, weights, pkg):
    W = weights["primary"]
    with pytest.raises(pkg.PfhipError):
        run_logpow(ops, W, np.zeros(160 * 14 - 1, np.float32), [0], 13)
    with pytest.raises(pkg.PfhipError):
        run_logpow(ops, W, np.zeros(160 * 14 + 5, np.float32), [6], 13)


# ---- the P.808 net's input -----------------------------------------------------------------------------------------------------------
def melspec_f32(audio):
    """R.melspec as a float32 chain: the transform as a [321 -> 161] matrix product, every array and operation in float32."""
    k = np.arange(321)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * k / 321)
    ang = 2.0 * np.pi * ((k[:, None] * np.arange(161)[None, :]) % 321) / 321
    tr, ti = (win[:, None] * np.cos(ang)).astype(np.float32), (-win[:, None] * np.sin(ang)).astype(np.float32)
    y = np.pad(np.asarray(audio, np.float32), (160, 160))
    fr = y[np.arange(900)[:, None] * 160 + k[None, :]]
    re, im = fr @ tr, fr @ ti
    S = (re * re + im * im) @ R.mel_filters().T.astype(np.float32)
    assert S.dtype == np.float32
    db = np.float32(10) * np.log10(np.maximum(np.float32(1e-10), S)) - np.float32(10) * np.log10(np.maximum(np.float32(1e-10), S.max()))
    return (np.maximum(db, np.float32(-80)) + np.float32(40)) / np.float32(40)


def test_melspec_against_fp64(ops):
    """The mel input of the three golden windows in one call, against the float64 formulas of tests/dnsmos_ref.py (the recalled
    librosa settings) on the same float32 samples; silence is exactly 1 everywhere.

    Measured error / bound: tone plus noise 4.181e-06 / 1.313e-05, clipped square 7.809e-07 / 3.510e-06."""
    x = np.concatenate([R.case_window(c) for c in R.CASES])
    offs = [i * R.LEN_SAMPLES for i in range(3)]
    n = 3 * 900 * 120
    buf = out_with_canary(n)
    ops.dnsmos_melspec(dev(x), offs, out=buf)
    check_canary(buf, n)
    got = buf[:n].cpu().numpy().reshape(3, 900, 120)
    assert (got[1] == 1.0).all()
    for i, name in enumerate(R.CASES):
        w = x[offs[i]:offs[i] + R.MEL_SAMPLES]
        f64 = R.melspec(w)
        if name == "zeros":
            continue
        err, bound = report(f"melspec {name}", got[i], f64, melspec_f32(w))
        assert err <= bound
    s16 = np.round(x * 32768.0).astype(np.int16)
    assert np.array_equal(s16.astype(np.float32) / np.float32(32768.0), x)
    buf2 = out_with_canary(n)
    ops.dnsmos_melspec(dev(s16), offs, out=buf2)
    check_canary(buf2, n)
    assert bool((buf2[:n] == buf[:n]).all()), "s16 bits differ from f32 bits"


# ---- the head ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["primary", "p808"])
def test_globalmax_mlp_against_fp64(ops, weights, kind):
    """The real dense layers on random feature maps of 7 x 5 pixels whose maximum, for every other channel, sits in the last (odd) row.

    Measured error / bound: primary 1.406e-06 / 3.956e-06, P.808 1.276e-06 / 5.105e-06."""
    W, net = weights[kind], (R.PRIMARY if kind == "primary" else R.P808)
    rng = np.random.default_rng(11)
    N, H, Wd, C = 3, 7, 5, 64
    x = np.maximum(0.0, rng.normal(0.3, 1.0, (N, H, Wd, C))).astype(np.float32)
    x[:, H - 1, Wd - 1, ::2] = 6.0 + rng.random((N, C // 2)).astype(np.float32)
    names = [f"{net['prefix']}/{d}" for d in net["dense"]]
    mats = [W[f"{p}/MatMul/ReadVariableOp/resource:0"] for p in names]
    bias = [W[f"{p}/BiasAdd/ReadVariableOp/resource:0"] for p in names]
    D3 = mats[2].shape[1]
    buf = out_with_canary(N * D3)
    ops.globalmax_mlp(dev(x), dev(mats[0]), dev(bias[0]), dev(mats[1]), dev(bias[1]), dev(mats[2]), dev(bias[2]), out=buf)
    check_canary(buf, N * D3)
    got = buf[:N * D3].cpu().numpy().reshape(N, D3)
    h = torch.as_tensor(x).permute(0, 3, 1, 2)
    with torch.no_grad():
        f64, f32 = R.head(W, net, h.double(), torch.float64).numpy(), R.head(W, net, h, torch.float32).numpy()
    assert (x.max(axis=(1, 2))[:, ::2] >= 6.0).all()
    err, bound = report(f"globalmax_mlp {kind}", got, f64, f32)
    assert err <= bound


# ---- the networks, entry by entry, on their real weights -----------------------------------------------------------------------------
def net_through_ops(ops, W, net, h):
    """h: the first layer's input [N, H, W] on the device -> [N, D3] through conv3x3_relu (pool fused) and globalmax_mlp."""
    for name, pool in net["convs"]:
        h = ops.conv3x3_relu(h, dev(W[f"{name}/kernel:0"]), dev(W[f"{name}/bias:0"]), pool=pool)
    names = [f"{net['prefix']}/{d}" for d in net["dense"]]
    args = []
    for p in names:
        args += [dev(W[f"{p}/MatMul/ReadVariableOp/resource:0"]), dev(W[f"{p}/BiasAdd/ReadVariableOp/resource:0"])]
    return ops.globalmax_mlp(h, *args).cpu().numpy()


def check_against_cases(what, got, f64, f32):
    """Within max(8 x the fixture's worst |fp32 - fp64|, 16 float32 ulp at the output's magnitude) of the float64 value."""
    bound = np.maximum(8 * np.abs(f32.astype(np.float64) - f64).max(), 16 * np.spacing(np.abs(f64).astype(np.float32)).astype(np.float64))
    err = np.abs(got.astype(np.float64) - f64)
    print(f"{what}: worst error {err.max():.3e}  bound {bound.min():.3e}")
    assert (err <= bound).all()


def test_primary_net_on_real_weights(ops, weights, cases):
    """The three golden windows through logpow, the seven convolutions and the head, on the file's own weights, against
    dnsmos_cases.npz.  Measured worst error / smallest bound: 1.116e-06 / 8.235e-06."""
    W = weights["primary"]
    x = np.concatenate([R.case_window(c) for c in R.CASES])
    h = ops.dnsmos_logpow(dev(x), [i * R.LEN_SAMPLES for i in range(3)], dev(W["time2freq/stft-real/kernel:0"]),
                          dev(W["time2freq/stft-imag/kernel:0"]))
    got = net_through_ops(ops, W, R.PRIMARY, h)
    check_against_cases("primary net", got, cases["primary_f64"], cases["primary_f32"])


def test_p808_net_on_real_weights(ops, weights, cases):
    """The same for model_v8's weights from the mel input.  Measured worst error / smallest bound: 2.171e-07 / 3.815e-06."""
    W = weights["p808"]
    x = np.concatenate([R.case_window(c) for c in R.CASES])
    h = ops.dnsmos_melspec(dev(x), [i * R.LEN_SAMPLES for i in range(3)])
    got = net_through_ops(ops, W, R.P808, h)
    check_against_cases("p808 net", got, cases["p808_f64"], cases["p808_f32"])
