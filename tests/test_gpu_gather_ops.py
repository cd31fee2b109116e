"""GPU: the row gathers and small reductions that only whole-model tests reached (compact, gather_rows, svs_prompt_rows, gather_best,
row_lse, argmax_first), each through its own operator entry (include/pfhip_ops.h).  The gathers and the arg-max are exact: outputs
start as a canary and are compared bit for bit, written region and the rest.  row_lse is compared with an fp64 log-sum-exp under a
derived bound.  Conventions of tests/test_gpu_row_ops.py.
"""
import importlib

import numpy as np
import pytest

import frontend_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32, F64 = np.float32, np.float64
CANARY = F32(-1234.5)
WIDTHS = [4, 320, 512, 516]          # one float4; the small and the large Paraformer; four channels past the 128-thread block's 512


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def canary(shape):
    return torch.full(shape, float(CANARY), dtype=torch.float32, device="cuda")


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def report(name, err, bound):
    """Largest error over bound (elements whose bound is 0 must have no error); printed, returned for the assertion."""
    err, bound = np.asarray(err, F64), np.asarray(bound, F64)
    assert np.all(err[bound == 0] == 0), f"{name}: an error where the bound is zero"
    ratio = float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0
    print(f"{name}: max err / bound = {ratio:.3f} (max abs err {float(err.max()) if err.size else 0.0:.3e})")
    return ratio


@pytest.mark.parametrize("D", WIDTHS)
def test_compact_and_gather_rows(ops, D):
    """emb[r] = stage[src_row[r]] and out[r] = table[ids[r]]: rows repeated, first and last row of the source, out of order; the rows
    after the last one keep the canary."""
    rng = np.random.default_rng(D)
    src = rng.standard_normal((19, D)).astype(F32)
    idx = np.array([18, 0, 0, 7, 18, 3, 11], np.int32)
    for fn in (ops.compact, ops.gather_rows):
        out = canary((len(idx) + 2, D))
        if fn is ops.compact:
            ops.compact(dev(src), out, dev(idx), len(idx), D)
        else:
            ops.gather_rows(dev(idx), dev(src), D, out, len(idx))
        got = host(out)
        assert same_bits(got[:len(idx)], src[idx]) and np.all(bits(got[len(idx):]) == bits(CANARY))
    out = canary((3, D))
    ops.compact(dev(src), out, dev(idx), 0, D)              # no rows: nothing is written
    ops.gather_rows(dev(idx), dev(src), D, out, 0)
    assert np.all(bits(host(out)) == bits(CANARY))


def test_gathers_refuse_widths_that_are_no_float4(ops, pkg):
    """The kernels copy float4s: D % 4 != 0 is refused by the entry before anything is launched."""
    src, idx, out = dev(np.zeros((4, 8), F32)), dev(np.zeros(2, np.int32)), canary((2, 8))
    for D in (0, 1, 6, 7):
        with pytest.raises(pkg.PfhipError):
            ops.compact(src, out, idx, 2, D)
        with pytest.raises(pkg.PfhipError):
            ops.gather_rows(idx, src, D, out, 2)
        with pytest.raises(pkg.PfhipError):
            ops.svs_prompt_rows(src, D, idx, idx, idx, 1, out)
    with pytest.raises(pkg.PfhipError):
        ops.svs_prompt_rows(src, 8, idx, idx, idx, 1, out[:, :4].contiguous())       # ld below D
    assert np.all(bits(host(out)) == bits(CANARY))


@pytest.mark.parametrize("D", WIDTHS)
def test_svs_prompt_rows(ops, D):
    """Rows row_off[b] .. + 3 of feats = rows prompt[4 b ..] of E for utterances of 4 rows and more; an utterance with len < 4 (0, 3) is
    left untouched, and so are every other row and the pad columns D .. ld."""
    rng = np.random.default_rng(D + 1)
    E = rng.standard_normal((16, D)).astype(F32)
    length = np.array([9, 3, 4, 0, 5], np.int32)
    row_off = np.array([0, 9, 12, 16, 16], np.int32)
    prompt = rng.integers(0, 16, 4 * len(length)).astype(np.int32)
    prompt[0], prompt[1] = 15, 0
    ld = D + 4
    feats = canary((int(length.sum()) + 2, ld))
    ops.svs_prompt_rows(dev(E), D, dev(prompt), dev(row_off), dev(length), len(length), feats)
    want = np.full(feats.shape, CANARY, F32)
    for b in range(len(length)):
        if length[b] >= 4:
            want[row_off[b]:row_off[b] + 4, :D] = E[prompt[4 * b:4 * b + 4]]
    assert same_bits(host(feats), want)


@pytest.mark.parametrize("M", [1, 256, 257])
def test_gather_best(ops, M):
    """best[r] = logp[r][ids[r]], exact: first and last column among the ids, ld above V, two blocks of rows at M = 257."""
    rng = np.random.default_rng(M)
    V, ld = 37, 40
    logp = rng.standard_normal((M, ld)).astype(F32)
    ids = rng.integers(0, V, M).astype(np.int32)
    ids[0], ids[-1] = V - 1, 0
    best = canary((M + 3,))
    ops.gather_best(dev(logp), dev(ids), M, best)
    got = host(best)
    assert same_bits(got[:M], logp[np.arange(M), ids]) and np.all(bits(got[M:]) == bits(CANARY))


@pytest.mark.parametrize("V", [1, 63, 64, 65, 25055])
def test_row_lse(ops, V):
    """lse[r] against the fp64 log-sum-exp.  Rows: within +-10, all equal, near +-80 (half at +80, half at -80 within 1), some -inf
    entries, a single finite entry, and a row all -inf, which gives -inf exactly; ld above V with +100 in the pad columns; M = 6 rows,
    two blocks of four.  Bound (tests/test_gpu_row_ops.py's softmax bound carried through the log): the sum's relative error
    (sum_c p_c |x_c - m| + V / 64 + 16) * 2^-23 with p the softmax shares, plus 4 ulp of log(sum) for logf, plus one ulp of the result.
    Measured on the MI355X: max err / bound = 0.307 (V = 63; 0.000 at 1, 0.127 at 64, 0.227 at 65, 0.021 at 25055)."""
    rng = np.random.default_rng(V)
    M, ld = 6, V + 3
    x = np.full((M, ld), 100.0, F32)
    x[0, :V] = rng.uniform(-10, 10, V)
    x[1, :V] = F32(rng.uniform(-10, 10))
    x[2, :V] = np.where(np.arange(V) % 2 == 0, 80.0, -80.0) + rng.uniform(-1, 1, V)
    x[3, :V] = rng.uniform(-10, 10, V)
    x[3, :V][rng.random(V) < 0.5] = -np.inf
    x[3, V - 1] = 3.0                                        # (at least one finite entry)
    x[4, :V] = -np.inf
    x[4, V // 2] = -7.25
    x[5, :V] = -np.inf
    lse = canary((M + 3,))
    ops.row_lse(dev(x), M, V, lse)
    got = host(lse)
    assert np.all(bits(got[M:]) == bits(CANARY))
    assert got[5] == -np.inf
    xd = x[:5, :V].astype(F64)
    ref = R.logsumexp64(xd)
    m = xd.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        p = np.exp(xd - ref[:, None])
        dist = np.where(np.isfinite(xd), p * np.abs(xd - m), 0.0).sum(axis=1)
    bound = (dist + V / 64.0 + 16.0) * 2.0 ** -23 + 4 * R.ulp32(ref - m[:, 0]) + R.ulp32(ref)
    assert report(f"row_lse V = {V}", np.abs(got[:5].astype(F64) - ref), bound) <= 1.0


@pytest.mark.parametrize("N,ncls,ldl", [(257, 5, 128), (7, 1, 128), (300, 128, 128), (5, 6, 8)])
def test_argmax_first(ops, N, ncls, ldl):
    """First-maximum semantics (std::max_element): ties take the lowest column, all-equal rows give 0, ncls = 1 gives 0, columns
    ncls .. ldl (which hold the largest values) are ignored, a NaN outside column 0 never wins; N = 257 is two blocks."""
    rng = np.random.default_rng(N + ncls)
    x = rng.standard_normal((N, ldl)).astype(F32)
    x[:, ncls:] = 1000.0
    want = np.argmax(x[:, :ncls], axis=1).astype(np.int32)
    for r in range(0, N, 3):                                # a tie of the maximum at two columns: the first wins
        if ncls >= 2:
            a, b = sorted(rng.choice(ncls, 2, replace=False))
            x[r, :ncls] = np.minimum(x[r, :ncls], 0.5)
            x[r, a] = x[r, b] = 2.0
            want[r] = a
    x[1 % N, :ncls] = -3.5                                  # all equal
    want[1 % N] = 0
    if ncls >= 3 and N > 4:
        x[4, :ncls] = [0.1 * c for c in range(ncls)]
        x[4, ncls - 1] = np.nan                             # would be the maximum's place; the NaN is skipped
        want[4] = ncls - 2
        x[2, :ncls] = -1.0
        x[2, 1] = np.nan                                    # a NaN before the maximum
        x[2, ncls - 1] = 4.0
        want[2] = ncls - 1
    out = torch.full((N + 3,), -7, dtype=torch.int32, device="cuda")
    ops.argmax_first(dev(x), N, ncls, out)
    got = host(out)
    assert np.array_equal(got[:N], want) and np.all(got[N:] == -7)


def test_reduction_refusals(ops, pkg):
    x, out = dev(np.zeros((4, 8), F32)), canary((4,))
    iout = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    for V in (0, 9):
        with pytest.raises(pkg.PfhipError):
            ops.row_lse(x, 4, V, out)
        with pytest.raises(pkg.PfhipError):
            ops.argmax_first(x, 4, V, iout)
    with pytest.raises(pkg.PfhipError):
        ops.gather_best(x, None, 4, out)
    assert np.all(bits(host(out)) == bits(CANARY)) and np.all(host(iout) == -7)
