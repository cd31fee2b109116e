"""GPU: the head with N-best candidates (csrc/topk.hip) through pfhip_op_logsoftmax_topk.

Ids are compared exactly with np.lexsort((column, -logit)) (larger logit first, equal logits smaller column first: FindMax's rule,
util.cpp:63-74), values bitwise with the same launch's own logp rows and, within the tolerance the head test of test_gpu_ops.py
uses for logp (1e-5), with an fp64 log-softmax.  The rows are the smallest that break a wrong merge; see make_rows."""
import functools
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

M = 5
SHAPES = [(8404, 8448), (257, 257), (33, 40), (8, 8)]      # 16-byte path (padded rows), scalar path, a row shorter than one thread stride
LOGP_TOL = 1e-5                                            # tests/test_gpu_ops.py::test_logsoftmax_argmax_first_max_wins


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()         # make_rows' arrays are shared and read-only


def thread_columns(t, V, ld):
    """Columns thread t of the 256-thread block reads, in its own order: c4 = t, t + 256, ... (four columns each) on the 16-byte path,
    c = t, t + 256, ... on the scalar path.  The leading column of every 16-byte group comes first (4 (t + 256 j) of the issue)."""
    if V % 4 == 0 and ld % 4 == 0:
        lead = [4 * c4 for c4 in range(t, V // 4, 256)]
        return lead + [c + i for c in lead for i in (1, 2, 3)]
    return list(range(t, V, 256))


@functools.lru_cache(maxsize=None)
def make_rows(V, ld):
    """[M, ld] logits (pad columns hold 100: they must be ignored) and, computed once, the fp64 log-softmax of the V columns.
    row 0  finite normal x 4
    row 1  the 8 largest values all in ONE thread's columns, planted out of order (a per-thread list shorter than k loses some)
    row 2  equal maxima at columns 3, 4000 and 8403 (V = 8404; 3, V // 2, V - 1 otherwise): ties inside the merge across lanes / waves
    row 3  all logits equal: the candidates are columns 0..k-1
    row 4  two distinct logits one ulp apart whose logp round equal, the larger at the larger column: the order follows the logit"""
    rng = np.random.default_rng(1000 + V)
    x = (4.0 * rng.standard_normal((M, ld))).astype(np.float32)
    own = thread_columns(5 if V > 2048 else 0, V, ld)[:8]      # thread 0 of a short row: the only one with more than one column
    x[1, :V] = np.minimum(x[1, :V], 10.0)
    x[1, own] = (12.0 + 0.5 * rng.permutation(len(own))).astype(np.float32)
    tie = [3, 4000, 8403] if V == 8404 else [3, V // 2, V - 1]
    x[2, :V] = np.minimum(x[2, :V], 20.0)
    x[2, tie] = 30.0
    x[3, :V] = -5.0
    hi = np.float32(1e-3)
    x[4, :V] = x[4, :V] - 40.0
    x[4, 1], x[4, V - 2] = np.nextafter(hi, np.float32(-1.0)), hi
    assert x[4, 1] < x[4, V - 2]
    x[:, V:] = 100.0
    z = x[:, :V].astype(np.float64)
    z = z - z.max(-1, keepdims=True)
    ref = z - np.log(np.exp(z).sum(-1, keepdims=True))
    x.setflags(write=False); ref.setflags(write=False)
    return x, ref


def expected_ids(x, V, k):
    col = np.arange(V)
    return np.stack([np.lexsort((col, -x[r, :V]))[:k] for r in range(x.shape[0])]).astype(np.int32)


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("V,ld", SHAPES)
def test_topk_ids_and_values(ops, V, ld, k):
    x, ref = make_rows(V, ld)
    logp, ids, tk_ids, tk_logp = [t.cpu().numpy() for t in ops.logsoftmax_topk(dev(x), k, V=V)]
    want = expected_ids(x, V, k)
    print(f"V={V} ld={ld} k={k}: id mismatches {(tk_ids != want).sum()}, max |logp - fp64| "
          f"{np.abs(tk_logp - np.take_along_axis(ref, want.astype(np.int64), 1)).max():.3e}")
    assert np.array_equal(tk_ids, want)
    assert np.array_equal(tk_ids[3], np.arange(k))                              # all-equal row
    assert tk_ids[4, 0] == V - 2 and (k == 1 or tk_ids[4, 1] == 1)              # the order follows the logit ...
    assert logp[4, V - 2] == logp[4, 1]                                         # ... where the log-probabilities round equal
    # candidate 0 is the arg-max id, and the ids are the existing kernel's on the same logits
    assert np.array_equal(tk_ids[:, 0], ids)
    _, ids0 = ops.logsoftmax_argmax(dev(x), V=V, want_logp=False)
    assert np.array_equal(ids, ids0.cpu().numpy())
    # values: bit for bit the launch's own logp entries; the fp64 log-softmax within the head test's tolerance; descending
    own = np.take_along_axis(logp, tk_ids.astype(np.int64), 1)
    assert np.array_equal(tk_logp.view(np.int32), own.view(np.int32))
    assert np.abs(tk_logp - np.take_along_axis(ref, tk_ids.astype(np.int64), 1)).max() < LOGP_TOL
    assert (np.diff(tk_logp, axis=1) <= 0).all()
    # the existing kernel writes the same logp bits
    logp0, _ = ops.logsoftmax_argmax(dev(x), V=V)
    assert np.array_equal(logp.view(np.int32), logp0.cpu().numpy().view(np.int32))
    # logp = NULL: the log-sum-exp pass still runs; the same candidates bit for bit
    none, ids_n, tk_ids_n, tk_logp_n = ops.logsoftmax_topk(dev(x), k, V=V, want_logp=False)
    assert none is None
    assert np.array_equal(ids_n.cpu().numpy(), ids) and np.array_equal(tk_ids_n.cpu().numpy(), tk_ids)
    assert np.array_equal(tk_logp_n.cpu().numpy().view(np.int32), tk_logp.view(np.int32))


@pytest.mark.parametrize("V,k", [(7, 8), (8404, 0), (8404, 9)])
def test_topk_refused_before_launch(ops, pkg, V, k):
    """V < k and k outside 1..8: hipErrorInvalidValue (1), and no buffer is written."""
    lib = ops._lib()
    x = dev(np.zeros((M, 8448), np.float32))
    ids = torch.full((M,), -7, dtype=torch.int32, device="cuda")
    tk_ids = torch.full((M, 8), -7, dtype=torch.int32, device="cuda")
    tk_logp = torch.full((M, 8), -7.0, dtype=torch.float32, device="cuda")
    rc = lib.pfhip_op_logsoftmax_topk(ops._p(x), 8448, M, V, k, None, ops._p(ids), ops._p(tk_ids), ops._p(tk_logp), ops._stream())
    torch.cuda.synchronize()
    assert rc == 1
    assert (ids == -7).all() and (tk_ids == -7).all() and (tk_logp == -7.0).all()
    with pytest.raises(pkg.PfhipError):
        ops.logsoftmax_topk(x, k, V=V)
