"""GPU: the gathered emissions of the CTC aligner (csrc/ctc_align.hip) through pfhip_op_ctc_emissions, against float64.

E_b[t][j] = x_t . W[id_j] + bias[id_j] - lse[row]: a grouped GEMM whose B operand is a gather of rows of W.  The kernel works on
64 x 64 tiles with a K-step of 32, so the cases put n_lab + 1 and len on both sides of one and two tiles, take the last row of W and a
label that occurs three times, K = 32 (one step) and K = 512, and a ragged batch with an utterance of no rows.  E is filled with a
sentinel and has slack at both ends: nothing but the utterances' own entries may change.

Tolerance, as tests/test_gpu_ctc_head_op.py sets its own: the same entries are formed on the same inputs by the route the project
already has (the fp16 two-plane GEMM of pfhip_op_gemm_f32_kind, kind 9, over ALL V columns, then pfhip_op_logsoftmax_argmax), both
errors against float64 are printed, and the new one may be at most twice the existing one."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V = 1003
BLANK = 0
SENTINEL = np.float32(-12345.0)
SLACK = 37


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def labels_of(rng, n):
    """n labels in 1 .. V - 1 with label V - 1 present and one id three times (where n allows)."""
    y = [int(x) for x in rng.integers(1, V, size=n)]
    if n >= 1:
        y[n // 2] = V - 1
    if n >= 5:
        y[0] = y[2] = y[4] = 17
    return y


def check(ops, K, lens, n_labs, seed):
    rng = np.random.default_rng(seed)
    B = len(lens)
    gaps = [3, 0, 5, 1, 2, 4, 0, 6][:B]                              # rows between utterances that belong to nobody
    row_off, M = [], 0
    for b in range(B):
        M += gaps[b]
        row_off.append(M)
        M += lens[b]
    M += 2
    X = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((V, K)) / np.sqrt(K)).astype(np.float32)
    bias = (0.02 * rng.standard_normal(V)).astype(np.float32)
    labels = [labels_of(rng, n) for n in n_labs]
    logits64 = X.astype(np.float64) @ W.astype(np.float64).T + bias.astype(np.float64)
    mx = logits64.max(axis=1, keepdims=True)
    lse64 = mx[:, 0] + np.log(np.exp(logits64 - mx).sum(axis=1))
    lse = lse64.astype(np.float32)

    Xd, Wd, bd, lsed = (torch.from_numpy(a).cuda() for a in (X, W, bias, lse))
    lab = ops.CtcLabels(labels, lens)
    Ed = torch.full((lab.e_floats + 2 * SLACK,), float(SENTINEL), dtype=torch.float32, device="cuda")
    ops.ctc_emissions(Xd, Wd, bd, lsed, torch.tensor(row_off, dtype=torch.int32, device="cuda"), lab, blank=BLANK, E=Ed, e_base=SLACK)
    # the existing unfused route on the same operands (padded as that GEMM wants them)
    ws = ops.best_w_scale(float(np.abs(W).max()))
    Mp, Vp = ops.round_up(M, 128), ops.round_up(V, 128)
    Xp = torch.zeros((Mp, K), dtype=torch.float32, device="cuda"); Xp[:M] = Xd
    Wp = torch.zeros((Vp, K), dtype=torch.float32, device="cuda"); Wp[:V] = Wd
    bp = torch.zeros(Vp, dtype=torch.float32, device="cuda"); bp[:V] = bd
    logits = ops.gemm_f32(Xp, Wp, bias=bp, M=M, N=V, guard=True, kind=9, w_scale=ws)
    ulogp, _ = ops.logsoftmax_argmax(logits[:M], V=V)
    torch.cuda.synchronize()
    E = Ed.cpu().numpy()
    ulogp = ulogp.cpu().numpy()

    assert (E[:SLACK] == SENTINEL).all() and (E[SLACK + lab.e_floats:] == SENTINEL).all(), "written outside E"
    body = E[SLACK:SLACK + lab.e_floats]
    assert not (body == SENTINEL).any(), "an entry of E was not written"
    err_new = err_old = 0.0
    for b in range(B):
        if lens[b] == 0:
            continue
        cols = [BLANK] + labels[b]
        rows = np.arange(row_off[b], row_off[b] + lens[b])
        want = logits64[np.ix_(rows, cols)] - lse64[rows][:, None]
        got = lab.cut(body, b)
        err_new = max(err_new, float(np.abs(got - want).max()))
        err_old = max(err_old, float(np.abs(ulogp[np.ix_(rows, cols)] - want).max()))
    print(f"K {K}, len {lens}, n_lab {n_labs}: max abs error against float64: gathered emissions {err_new:.3e}, "
          f"GEMM + log-softmax {err_old:.3e}")
    assert err_new <= 2.0 * err_old, (err_new, err_old)


@pytest.mark.parametrize("K", [32, 512])
@pytest.mark.parametrize("C", [1, 2, 128, 129])
def test_label_counts_around_the_tiles(ops, K, C):
    check(ops, K, [70], [C - 1], seed=1000 + C + K)


@pytest.mark.parametrize("K", [32, 512])
@pytest.mark.parametrize("N", [1, 127, 128, 129])
def test_lengths_around_the_tiles(ops, K, N):
    check(ops, K, [N], [9], seed=2000 + N + K)


@pytest.mark.parametrize("K", [32, 512])
def test_ragged_batch(ops, K):
    check(ops, K, [129, 0, 1, 65, 200], [130, 4, 0, 64, 7], seed=3000 + K)


def test_refused_before_launch(ops, pkg):
    X, W, b, lse = (torch.zeros(s, dtype=torch.float32, device="cuda") for s in ((4, 48), (8, 48), (8,), (4,)))
    lab = ops.CtcLabels([[1, 2]], [4])
    off = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(pkg.PfhipError):
        ops.ctc_emissions(X, W, b, lse, off, lab)                    # K % 32 != 0
    X, W = (torch.zeros(s, dtype=torch.float32, device="cuda") for s in ((4, 64), (8, 64)))
    with pytest.raises(pkg.PfhipError):
        ops.ctc_emissions(X, W, b, lse, off, lab, blank=8)           # the blank is no row of W
    with pytest.raises(pkg.PfhipError):
        ops.ctc_emissions(X, W, b, None, off, lab)                   # NULL log-sum-exp
    torch.cuda.synchronize()
