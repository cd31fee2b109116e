"""GPU: the plan kernel of the in-forward greedy alignment on its own (pfhip_op_ctc_greedy_plan, csrc/ctc_align.hip): from the
collapse's token_num [B] and the speech rows N_b it forms n_lab, lab_off and the exclusive int64 prefix sums e_off on the device.
Everything is integer arithmetic, so every value is pinned EXACTLY against numpy int64.  B = 1 and 3 (less than a wave), 70 (crosses a
wave), 300 (more utterances than the workgroup has threads: the scan's second chunk and its carry)."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MAXT = 37
SENTINEL = -77                      # what ops.ctc_greedy_plan pre-fills its outputs with


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def plan_ref(token_num, speech_len, maxT, cap):
    """include/pfhip_ops.h's statement, in numpy int64."""
    tn, N = np.asarray(token_num, np.int64), np.asarray(speech_len, np.int64)
    B = len(tn)
    n_lab = np.maximum(tn - 4, 0)
    bad = (tn > maxT) | (N < 0)
    size = np.where(bad, 0, N * (n_lab + 1))
    e_off = np.concatenate([[0], np.cumsum(size)])[:-1].astype(np.int64) if B else np.zeros(0, np.int64)
    n_lab = np.where(bad | (e_off + size > cap), -1, n_lab)
    lab_off = np.arange(B, dtype=np.int64) * maxT + 4
    return n_lab, lab_off, e_off, int(size.sum())


def inputs(B, seed):
    """token_num cycles through 0, 3, 4, 5 and maxT (no token, fewer than the tags, the tags alone, one text token, a full row) and
    random counts; the speech rows include 0 and are otherwise at least the text tokens, as a collapse leaves them."""
    rng = np.random.default_rng(seed)
    fixed = [0, 3, 4, 5, MAXT]
    tn = np.array([fixed[b % 5] if b % 2 == 0 else int(rng.integers(0, MAXT + 1)) for b in range(B)], np.int32)
    N = np.array([0 if b % 7 == 3 else int(max(tn[b] - 4, 0) + rng.integers(0, 600)) for b in range(B)], np.int32)
    return tn, N


def run(ops, tn, N, maxT, cap):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    n_lab, lab_off, e_off, total = ops.ctc_greedy_plan(dev(tn), dev(N), maxT, cap)
    torch.cuda.synchronize()
    return n_lab.cpu().numpy().astype(np.int64), lab_off.cpu().numpy().astype(np.int64), e_off.cpu().numpy(), int(total.item())


def check(ops, tn, N, maxT, cap):
    got, want = run(ops, tn, N, maxT, cap), plan_ref(tn, N, maxT, cap)
    for name, g, w in zip(("n_lab", "lab_off", "e_off"), got, want):
        assert g.tolist() == w.tolist(), name
    assert got[3] == want[3]
    return got


@pytest.mark.parametrize("B", [1, 3, 70, 300])
def test_plan_equals_numpy_int64(ops, B):
    tn, N = inputs(B, 100 + B)
    n_lab, _, e_off, total = check(ops, tn, N, MAXT, 1 << 40)
    assert (n_lab >= 0).all() and total == int((N.astype(np.int64) * (n_lab + 1)).sum())
    if B >= 70:
        assert {0, 3, 4, 5, MAXT} <= set(tn.tolist()) and (N == 0).any() and total > 0


@pytest.mark.parametrize("B", [3, 70, 300])
def test_the_last_two_do_not_fit(ops, B):
    """A capacity one float short of the last-but-one utterance's end: that one and the last get n_lab -1, every other value — the
    refused ones' e_off and the total included — is what a capacity without a limit gives."""
    tn, N = inputs(B, 200 + B)
    tn[-2:], N[-2:] = [9, 6], [40, 11]                     # both have rows and text tokens
    free = plan_ref(tn, N, MAXT, 1 << 40)
    cap = int(free[2][-2] + 40 * 6 - 1)
    n_lab, lab_off, e_off, total = check(ops, tn, N, MAXT, cap)
    assert n_lab[-2:].tolist() == [-1, -1]
    assert n_lab[:-2].tolist() == free[0][:-2].tolist() and (n_lab[:-2] >= 0).all()
    assert e_off.tolist() == free[2].tolist() and total == free[3]
    # one float more and the last-but-one fits again
    assert run(ops, tn, N, MAXT, cap + 1)[0][-2:].tolist() == [5, -1]


def test_counts_no_collapse_leaves_are_refused(ops):
    """token_num above maxT (its labels would lie outside the utterance's row of the id buffer) and a negative row count: n_lab -1 and
    nothing added to the sums; the neighbours are served."""
    tn = np.array([10, MAXT + 1, 8, 12, 6], np.int32)
    N = np.array([20, 50, -3, 30, 2], np.int32)
    n_lab, _, e_off, total = check(ops, tn, N, MAXT, 1 << 40)
    assert n_lab.tolist() == [6, -1, -1, 8, 2]
    assert e_off.tolist() == [0, 140, 140, 140, 410] and total == 416


def test_arguments_are_refused_before_the_launch(pkg, ops):
    tn = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(pkg.PfhipError):
        ops.ctc_greedy_plan(tn, tn, -1, 100)
    with pytest.raises(pkg.PfhipError):
        ops.ctc_greedy_plan(tn, tn, MAXT, -1)
    with pytest.raises(pkg.PfhipError):
        ops.ctc_greedy_plan(tn, tn, 1 << 30, 100)          # 3 * maxT + 4 does not fit an int
