"""GPU: the fused CTC head with the k best columns of every row (csrc/ctc_head.hip) through pfhip_op_ctc_head_topk, K = 512, against
a float64 head.  Operands are those of tests/test_gpu_ctc_head_op.py (its `operands`): (M, V) = (200, 300), (130, 129), (200, 1200),
the +-80 logits and the equal-maxima case; k in {1, 3, 10, 16}.

Checks: rank 0 — ids, logp_best, lse and the first top-k column — equals pfhip_op_ctc_head on the same operands BIT FOR BIT; a
row's values do not increase and no column occurs twice; per rank the rule and the numbers of the greedy test: where the device's
column differs from float64's at that rank it must be float64's neighbour in rank with a float64 gap below 1e-4, for at most 0.5 %
of the (row, rank) pairs of a case; the value error against float64 is at most twice that of the unfused path (the fp16 two-plane
GEMM, kind 9, then pfhip_op_logsoftmax_argmax) on the same entries.  Both errors are printed."""
import functools
import importlib

import numpy as np
import pytest

from test_gpu_ctc_head_op import K, TIE_GAP, TIE_SHARE, operands

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KMAX = 16


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64: (logits - lse [M, V], the 17 best columns of every row in rank order — stable, the lower column first among equals)."""
    X, W, b = operands(name)
    logits = X.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
    m = logits.max(axis=1, keepdims=True)
    logp = logits - (m + np.log(np.exp(logits - m).sum(axis=1, keepdims=True)))
    order = np.argsort(-logits, axis=1, kind="stable")[:, :KMAX + 1]
    logp.setflags(write=False); order.setflags(write=False)
    return logp, order


@functools.lru_cache(maxsize=None)
def device_baseline(name):
    """The greedy fused head (bits to match) and the unfused path's log-softmax matrix (the error unit), once per case."""
    ops = importlib.import_module("asr_2pass_amd.ops")
    X, W, b = operands(name)
    M, V = X.shape[0], W.shape[0]
    Xd, Wd, bd = (torch.from_numpy(np.array(a, copy=True)).cuda() for a in (X, W, b))
    ws = ops.best_w_scale(float(np.abs(W).max()))
    ids, lp, lse = ops.ctc_head(Xd, Wd, bd, w_scale=ws)
    Mp, Vp = ops.round_up(M, 128), ops.round_up(V, 128)
    Xp = torch.zeros((Mp, K), dtype=torch.float32, device="cuda"); Xp[:M] = Xd
    Wp = torch.zeros((Vp, K), dtype=torch.float32, device="cuda"); Wp[:V] = Wd
    bp = torch.zeros(Vp, dtype=torch.float32, device="cuda"); bp[:V] = bd
    logits = ops.gemm_f32(Xp, Wp, bias=bp, M=M, N=V, guard=True, kind=9, w_scale=ws)
    ulogp, _ = ops.logsoftmax_argmax(logits[:M], V=V)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), lp.cpu().numpy(), lse.cpu().numpy(), ulogp.cpu().numpy()[:, :V].astype(np.float64), ws


def check(ops, name, k):
    X, W, b = operands(name)
    M, V = X.shape[0], W.shape[0]
    ref_logp, order = reference(name)
    g_ids, g_lp, g_lse, ulogp, ws = device_baseline(name)
    Xd, Wd, bd = (torch.from_numpy(np.array(a, copy=True)).cuda() for a in (X, W, b))
    ids, lp, lse, tk_ids, tk_lp = (t.cpu().numpy() for t in ops.ctc_head_topk(Xd, Wd, bd, k, w_scale=ws))
    # rank 0 is the greedy head, bit for bit
    assert np.array_equal(ids, g_ids) and np.array_equal(lp.view(np.uint32), g_lp.view(np.uint32))
    assert np.array_equal(lse.view(np.uint32), g_lse.view(np.uint32))
    assert np.array_equal(tk_ids[:, 0], g_ids) and np.array_equal(tk_lp[:, 0].view(np.uint32), g_lp.view(np.uint32))
    # well-formed rows
    assert tk_ids.shape == (M, k) and (tk_ids >= 0).all() and (tk_ids < V).all() and np.isfinite(tk_lp).all()
    assert (np.diff(tk_lp, axis=1) <= 0).all()
    assert all(len(set(r)) == k for r in tk_ids.tolist())
    # per rank: float64's column, or its neighbour in rank across a gap below 1e-4
    rows = np.arange(M)
    n_tie = 0
    for r in range(k):
        bad = np.nonzero(tk_ids[:, r] != order[:, r])[0]
        for i in bad:
            near = [q for q in (r - 1, r + 1) if 0 <= q <= KMAX and order[i, q] == tk_ids[i, r]]
            assert near, f"case {name} k {k} row {i} rank {r}: got column {tk_ids[i, r]}, float64 {order[i, max(r - 1, 0):r + 2]}"
            gap = abs(ref_logp[i, order[i, r]] - ref_logp[i, tk_ids[i, r]])
            assert gap < TIE_GAP, f"case {name} k {k} row {i} rank {r}: float64 gap {gap:.2e}"
        n_tie += len(bad)
    assert n_tie <= TIE_SHARE * M * k, f"case {name} k {k}: {n_tie} of {M * k} (row, rank) pairs needed the tie rule"
    # values: each against float64's value of the device's own column; the unfused path on float64's k best columns
    err_fused = float(np.abs(tk_lp - ref_logp[rows[:, None], tk_ids]).max())
    err_unfused = float(np.abs(ulogp[rows[:, None], order[:, :k]] - ref_logp[rows[:, None], order[:, :k]]).max())
    print(f"case {name} k {k}: value max abs error against float64: fused {err_fused:.3e}, unfused {err_unfused:.3e}; "
          f"{n_tie} of {M * k} pairs on the tie rule")
    assert err_fused <= 2.0 * err_unfused, (name, k, err_fused, err_unfused)
    return tk_ids


@pytest.mark.parametrize("k", [1, 3, 10, 16])
def test_a_partial_row_and_column_tiles(ops, k):
    """M = 200, V = 300: two row tiles and three column tiles, the last with 44 columns (k = 16 takes entries from each)."""
    check(ops, "a", k)


@pytest.mark.parametrize("k", [3, 16])
def test_b129_k_above_the_valid_columns_of_the_last_tile(ops, k):
    """V = 129: the second tile has ONE valid column, fewer than k: its remaining pairs are empty and must not enter a row's list."""
    tk = check(ops, "b129", k)
    assert (tk < 129).all()


@pytest.mark.parametrize("k", [1, 10])
def test_g_ten_column_tiles(ops, k):
    """V = 1200: ten column tiles, a full column group of the tile order and a narrower one."""
    check(ops, "g", k)


def test_d_large_logits(ops):
    """Logits to +-80: the values stay finite and ordered."""
    check(ops, "d", 10)


@pytest.mark.parametrize("k", [3, 16])
def test_e_equal_maxima(ops, k):
    """Columns 5, 6 and 261 hold the same logit, the row's maximum: ranks 0-2 are exactly [5, 6, 261] — equal values inside a tile
    and across tiles come out lower column first."""
    tk = check(ops, "e", k)
    assert (tk[:, :3] == np.array([5, 6, 261])).all()


def test_refused_before_launch(ops, pkg):
    X, W, b = (torch.zeros(s, dtype=torch.float32, device="cuda") for s in ((4, 64), (8, 64), (8,)))
    for k in (0, 17, 9):                             # k = 0, k = 17, V = 8 < k = 9
        with pytest.raises(pkg.PfhipError):
            ops.ctc_head_topk(X, W, b, k, w_scale=1.0)
    with pytest.raises(pkg.PfhipError):
        ops.ctc_head_topk(X, W, b, 4, w_scale=1.0, workspace_bytes=16)
