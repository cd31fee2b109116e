"""GPU: the CTC head without the logits matrix (csrc/ctc_head.hip) through pfhip_op_ctc_head, K = 512, against a float64 head.

The kernel works on 128 x 128 tiles and merges a row's column tiles afterwards, so the cases are the smallest that reach every edge
of that: a partial row tile, a partial column tile, a column tile with ONE valid column, pad columns that would win or add to the
sum if they were not masked, logits of +-80 (the maximum must be subtracted before exp), equal maxima inside a tile and across
tiles, the maximum in the partial tile, and ten column tiles (a full column group of eight and a narrower one: the tile order).

ids: conftest.assert_ids_match's rule — the runner-up is accepted where the float64 top-2 gap is below 1e-4 — for at most 0.5 % of
the rows of a case.  logp_best: the same operands go through the unfused path the project already has (the fp16 two-plane GEMM of
pfhip_op_gemm_f32_kind, kind 9, with the same weight scale, then pfhip_op_logsoftmax_argmax); both errors against float64 are
printed and the fused one may be at most twice the unfused one (the tile merge reorders the sums, nothing else differs)."""
import functools
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K = 512
TIE_GAP = 1e-4
TIE_SHARE = 0.005


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


@functools.lru_cache(maxsize=None)
def operands(name):
    """(X [M, K], W [V, K], bias [V]) of a case: LayerNorm-like rows, N(0, 1/sqrt(K)) weights, small biases, then the case's edit."""
    M, V = {"a": (200, 300), "b128": (130, 128), "b129": (130, 129), "g": (200, 1200)}.get(name, (200, 300))
    rng = np.random.default_rng(sum(map(ord, name)))
    X = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((V, K)) / np.sqrt(K)).astype(np.float32)
    b = (0.02 * rng.standard_normal(V)).astype(np.float32)
    if name == "c":                     # every valid logit near -1e4: a pad column taken as 0 would win and own the sum
        b[:] = -1e4
    elif name == "d":                   # logits to +-80 (200 x 300 draws of N(0, 20^2): beyond 4 sigma)
        X *= np.float32(20.0)
    elif name == "e":                   # columns 5, 6 (same tile, neighbouring lanes) and 261 (tile 2, the lane of column 5) are one column
        W[6] = W[5]; W[261] = W[5]
        b[[5, 6, 261]] = 25.0
    elif name == "f":                   # the maximum in the last, partial tile: column 256 + row % 44 (10 x 3 = +30 on that logit)
        j = np.arange(44)
        W[256 + j, j] += np.float32(3.0)
        X[np.arange(M), np.arange(M) % 44] += np.float32(10.0)
    for a in (X, W, b):
        a.setflags(write=False)
    return X, W, b


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64: (ids, logp_best, top-2 gap, runner-up) per row."""
    X, W, b = operands(name)
    logits = X.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
    m = logits.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(logits - m).sum(axis=1))
    order = np.argsort(-logits, axis=1, kind="stable")          # stable: the lower column first among equals
    ids = order[:, 0]
    rows = np.arange(logits.shape[0])
    runner = order[:, 1] if logits.shape[1] > 1 else ids
    gap = logits[rows, ids] - logits[rows, runner]
    return ids, logits[rows, ids] - lse, gap, runner, lse


def run(ops, name):
    X, W, b = operands(name)
    M, V = X.shape[0], W.shape[0]
    Xd, Wd, bd = (torch.from_numpy(np.array(a, copy=True)).cuda() for a in (X, W, b))
    ws = ops.best_w_scale(float(np.abs(W).max()))
    ids, lp, lse = ops.ctc_head(Xd, Wd, bd, w_scale=ws)
    # the unfused path on the same operands (padded as that GEMM wants them)
    Mp, Vp = ops.round_up(M, 128), ops.round_up(V, 128)
    Xp = torch.zeros((Mp, K), dtype=torch.float32, device="cuda"); Xp[:M] = Xd
    Wp = torch.zeros((Vp, K), dtype=torch.float32, device="cuda"); Wp[:V] = Wd
    bp = torch.zeros(Vp, dtype=torch.float32, device="cuda"); bp[:V] = bd
    logits = ops.gemm_f32(Xp, Wp, bias=bp, M=M, N=V, guard=True, kind=9, w_scale=ws)
    ulogp, uids = ops.logsoftmax_argmax(logits[:M], V=V)
    torch.cuda.synchronize()
    uids = uids.cpu().numpy().astype(np.int64)
    ulp = ulogp.cpu().numpy()[np.arange(M), uids]
    return ids.cpu().numpy().astype(np.int64), lp.cpu().numpy(), lse.cpu().numpy(), uids, ulp


def check(ops, name, exact_ids=None):
    ref_ids, ref_lp, gap, runner, ref_lse = reference(name)
    ids, lp, lse, uids, ulp = run(ops, name)
    M = len(ref_ids)
    assert np.isfinite(lp).all() and np.isfinite(lse).all()
    if exact_ids is not None:
        assert ids.tolist() == list(exact_ids)
    bad = np.nonzero(ids != ref_ids)[0]
    for r in bad:
        assert gap[r] < TIE_GAP and ids[r] == runner[r], f"case {name} row {r}: got {ids[r]}, float64 {ref_ids[r]} (top-2 gap {gap[r]:.2e})"
    assert len(bad) <= TIE_SHARE * M, f"case {name}: {len(bad)} of {M} rows needed the tie rule"
    same = ids == ref_ids
    err_fused = float(np.abs(lp[same] - ref_lp[same]).max())
    usame = uids == ref_ids
    err_unfused = float(np.abs(ulp[usame] - ref_lp[usame]).max())
    err_lse = float(np.abs(lse - ref_lse).max())
    print(f"case {name}: logp_best max abs error against float64: fused {err_fused:.3e}, unfused {err_unfused:.3e}; lse {err_lse:.3e}; "
          f"{len(bad)} of {M} rows on the tie rule")
    assert err_fused <= 2.0 * err_unfused, (name, err_fused, err_unfused)
    return ids


def test_a_partial_row_and_column_tiles(ops):
    """M = 200: two row tiles, the second with 72 rows; V = 300: three column tiles, the last with 44 columns."""
    check(ops, "a")


@pytest.mark.parametrize("name", ["b128", "b129"])
def test_b_one_valid_column_in_a_tile(ops, name):
    """V = 128: exactly one full tile; V = 129: a second tile whose only valid column is 128.  M = 130: a row tile of two rows."""
    check(ops, name)


def test_c_pad_columns_neither_win_nor_add(ops):
    """Every bias -1e4: every valid logit is ~1e4 below what an unmasked pad column (bias read as 0, or W row V - 1 again) would hold."""
    ids = check(ops, "c")
    assert ids.max() < 300


def test_d_large_logits(ops):
    """Logits to +-80: exp of an unshifted logit would overflow fp32 at 88.7 and lose everything below; logp_best stays finite."""
    ref_ids, ref_lp, gap, runner, ref_lse = reference("d")
    assert np.abs(ref_lse).max() > 60
    check(ops, "d")


def test_e_equal_maxima(ops):
    """Columns 5, 6 and 261 hold the same logit, the row's maximum: the lowest column wins, inside a tile and across tiles."""
    check(ops, "e", exact_ids=[5] * 200)


def test_f_maximum_in_the_partial_tile(ops):
    """The maximum at column 256 + (row % 44), i.e. anywhere in the last tile (44 valid columns)."""
    check(ops, "f")
    ref_ids = reference("f")[0]
    assert (ref_ids >= 256).all() and len(set(ref_ids.tolist())) == 44


def test_g_ten_column_tiles(ops):
    """V = 1200: ten column tiles, more than the column group of the tile order (eight at K = 512), so the narrower last group runs."""
    check(ops, "g")


def test_refused_before_launch(ops, pkg):
    X, W, b = (torch.zeros(s, dtype=torch.float32, device="cuda") for s in ((4, 48), (8, 48), (8,)))
    with pytest.raises(pkg.PfhipError):
        ops.ctc_head(X, W, b, w_scale=1.0)          # K % 32 != 0
