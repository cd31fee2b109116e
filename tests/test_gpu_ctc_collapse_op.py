"""GPU: the CTC collapse kernel (csrc/ctc_head.hip) through pfhip_op_ctc_collapse, exact against a Python loop.

The loop restates CTCSearch (onnxruntime/src/sensevoice-small.cpp:331-343): a frame is kept when its id is not the blank and differs
from the previous frame's id.  The kernel scans an utterance in chunks of CHUNK = 256 frames (one frame per thread of the workgroup),
carrying the running count; lengths 255 / 256 / 257 and 1027 (four full chunks and three frames) sit on both sides of that width.
Every output is an integer or a copied float, so every comparison is exact; tok_logp is compared as bit patterns."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CHUNK = 256
BLANK = 0
LENGTHS = [1, 4, 5, 63, 64, 65, 255, 256, 257, 1027]


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    mod = importlib.import_module("asr_2pass_amd.ops")
    assert mod.ctc_collapse_chunk() == CHUNK          # the lengths above are chosen for this width
    return mod


def py_collapse(ids, blank=BLANK):
    """(kept ids, their frames) of one utterance."""
    out, frames, prev = [], [], -1
    for t, y in enumerate(int(v) for v in ids):
        if y != blank and y != prev:
            out.append(y)
            frames.append(t)
        prev = y
    return out, frames


def ctc_like_ids(n, rng):
    """Frame ids as a CTC head gives them: about half blank, about a quarter equal to their predecessor."""
    ids = np.where(rng.random(n) < 0.5, 0, rng.integers(1, 6, n)).astype(np.int32)
    rep = rng.random(n) < 0.25
    for t in range(1, n):
        if rep[t]:
            ids[t] = ids[t - 1]
    return ids


def run_and_check(ops, utts, seed, max_tokens=None, blank=BLANK):
    """One launch over the packed utterances; every output against the loop.  Returns token_num."""
    rng = np.random.default_rng(seed)
    lens = np.array([len(u) for u in utts], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    total = int(lens.sum())
    fid = np.concatenate([np.asarray(u, np.int32) for u in utts] + [np.zeros(1, np.int32)])[:max(total, 1)]
    flp = (-rng.random(max(total, 1)) * 5).astype(np.float32)
    want = [py_collapse(u, blank) for u in utts]
    cap = max([len(w[0]) for w in want] + [1]) if max_tokens is None else max_tokens
    ids, frames, logp, num = ops.ctc_collapse(torch.from_numpy(fid).cuda(), torch.from_numpy(flp).cuda(), torch.from_numpy(offs).cuda(),
                                              torch.from_numpy(lens).cuda(), cap, blank=blank)
    torch.cuda.synchronize()
    ids, frames, logp, num = ids.cpu().numpy(), frames.cpu().numpy(), logp.cpu().numpy(), num.cpu().numpy()
    for b, (wi, wf) in enumerate(want):
        assert int(num[b]) == len(wi), (b, int(num[b]), len(wi))
        n = min(len(wi), cap)
        assert ids[b, :n].tolist() == wi[:n], b
        assert frames[b, :n].tolist() == wf[:n], b
        src = flp[offs[b] + np.asarray(wf[:n], np.int64)] if n else np.zeros(0, np.float32)
        assert np.array_equal(logp[b, :n].view(np.int32), src.view(np.int32)), b          # a copy, bit for bit
        assert (ids[b, n:] == -1).all() and (frames[b, n:] == -1).all() and np.isnan(logp[b, n:]).all(), b      # nothing past the count
    return num


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths(ops, n):
    rng = np.random.default_rng(n)
    num = run_and_check(ops, [ctc_like_ids(n, rng)], seed=n)
    assert n < 60 or num[0] > 0


def test_all_blank(ops):
    num = run_and_check(ops, [np.zeros(300, np.int32)], seed=1)
    assert num[0] == 0


def test_no_blank_no_repeat(ops):
    ids = (np.arange(600) % 7 + 1).astype(np.int32)
    num = run_and_check(ops, [ids], seed=2)
    assert num[0] == 600


def test_run_across_chunk_boundary(ops):
    """One run of equal ids over frames 250..261 gives one token at frame 250, although its frames 256.. are scanned by another
    trip; a run that starts exactly at frame 512 is kept there."""
    ids = np.zeros(600, np.int32)
    ids[250:262] = 7
    ids[512:520] = 3
    num = run_and_check(ops, [ids], seed=3)
    assert num[0] == 2


def test_blank_separates_equal_ids(ops):
    """a _ a is two tokens, a a is one."""
    num = run_and_check(ops, [np.array([4, 0, 4], np.int32), np.array([4, 4], np.int32)], seed=4)
    assert num.tolist() == [2, 1]


def test_known_answers(ops):
    """a a _ a b b _ _ c -> a a b c; leading blanks; a blank as the very first frame."""
    a, b, c = 11, 12, 13
    num = run_and_check(ops, [np.array([a, a, 0, a, b, b, 0, 0, c], np.int32), np.array([0, 0, 0, a, a, b], np.int32),
                              np.array([0, a], np.int32)], seed=5)
    assert num.tolist() == [4, 2, 1]


def test_blank_id_is_a_parameter(ops):
    num = run_and_check(ops, [np.array([2, 0, 0, 2, 5], np.int32)], seed=6, blank=2)
    assert num[0] == 2


def test_empty_utterance_between_two(ops):
    rng = np.random.default_rng(7)
    num = run_and_check(ops, [ctc_like_ids(70, rng), np.zeros(0, np.int32), ctc_like_ids(300, rng)], seed=7)
    assert num[1] == 0


def test_seven_ragged_utterances(ops):
    rng = np.random.default_rng(8)
    run_and_check(ops, [ctc_like_ids(n, rng) for n in (513, 1, 0, 257, 64, 1027, 256)], seed=8)


def test_count_beyond_capacity(ops):
    """token_num is the true count when max_tokens is too small; the surplus is not stored (the next utterance's slots stay)."""
    ids = (np.arange(300) % 5 + 1).astype(np.int32)
    num = run_and_check(ops, [ids, ids[:3]], seed=9, max_tokens=40)
    assert num.tolist() == [300, 3]
