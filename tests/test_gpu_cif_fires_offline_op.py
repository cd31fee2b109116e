"""GPU: the offline CIF scan that also records where each token fired (csrc/cif.hip, cif_kernel<NC, true>) through
pfhip_op_cif_fires.

Everything is exact.  stage, n_fires and token_num are compared bit for bit with pfhip_op_cif's on the same inputs (the sibling runs
the same statements in the same order); fire_frame is compared with a numpy restatement of the kernel's loop that records the loop
index i of every fire (0..T-1 = an LFR row, T = the tail slot).  One packed batch of lengths 0, 1, 7, 8, 9 and 23 rows — they
straddle the kernel's 8-deep prefetch group — at D = 512 (NC = 1) and D = 520 (NC = 2), alphas in steps of 1/16 so that
alpha + integrate meets the threshold exactly, threshold 1.0 and tail 0.45 as in test_gpu_row_ops.
"""
import importlib

import numpy as np
import pytest

from test_gpu_row_ops import TAIL, THR, sixteenths

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32 = np.float32
LENS = [0, 1, 7, 8, 9, 23]
FIRE_CANARY = -99


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scan_fires(alphas, T, thr, tail):
    """The scalar part of cif_kernel's loop, statement for statement: the steps that fired, floor(sum alphas) with the tail's alpha
    in the sum as the kernel has it, and how often alpha + integrate met the threshold exactly."""
    integrate, asum = F32(0.0), F32(0.0)
    fires, exact = [], 0
    for i in range(T + 1):
        alpha = F32(alphas[i]) if i < T else F32(tail)
        asum = F32(asum + alpha)
        exact += int(F32(alpha + integrate) == thr)
        if F32(alpha + integrate) < thr:
            integrate = F32(integrate + alpha)
        else:
            fires.append(i)
            integrate = F32(integrate + alpha)
            integrate = F32(integrate - thr)
    return fires, int(np.floor(asum)), exact


def batch_alphas(rng):
    """Sixteenths, with the residue in front of the tail slot pinned for two utterances: the 7-row one ends on 10/16 (10/16 + 0.45
    fires the tail slot), the 8-row one on 2/16 (it does not).  The 9-row one starts with 1.0 and the 23-row one with 8/16, 8/16:
    alpha + integrate == threshold in rows 0 and 1, whatever the generator draws."""
    row_off = np.concatenate([[0], np.cumsum(LENS)[:-1]]).astype(np.int32)
    alphas = sixteenths(rng, int(sum(LENS)))
    alphas[row_off[4]] = 1.0
    alphas[row_off[5]:row_off[5] + 2] = 0.5
    for b, want in ((2, 10), (3, 2)):
        r, T = row_off[b], LENS[b]
        alphas[r + T - 1] = 0
        sixteenths_so_far = int(round(float(alphas[r:r + T].sum()) * 16))
        alphas[r + T - 1] = F32(((want - sixteenths_so_far) % 16) / 16.0)
    return row_off, alphas


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


@pytest.mark.parametrize("D", [512, 520])
def test_cif_fires_offline_exact(ops, D):
    rng = np.random.default_rng(2000 + D)
    B, M = len(LENS), int(sum(LENS))
    row_off, alphas = batch_alphas(rng)
    hidden = rng.standard_normal((M, D)).astype(F32)
    d_hidden, d_alphas, d_off, d_len = dev(hidden), dev(alphas), dev(row_off), dev(np.asarray(LENS, np.int32))
    stage_a, nf_a, tn_a = ops.cif(d_hidden, d_alphas, d_off, d_len, float(THR), float(TAIL))
    fire = torch.full((M + B,), FIRE_CANARY, dtype=torch.int32, device="cuda")
    stage_b, nf_b, tn_b, fire_out = ops.cif_fires(d_hidden, d_alphas, d_off, d_len, float(THR), float(TAIL), fire_frame=fire)
    assert fire_out is fire
    torch.cuda.synchronize()
    # the sibling's arithmetic is the default kernel's, bit for bit
    assert same_bits(stage_a.cpu().numpy(), stage_b.cpu().numpy())
    assert np.array_equal(nf_a.cpu().numpy(), nf_b.cpu().numpy())
    assert np.array_equal(tn_a.cpu().numpy(), tn_b.cpu().numpy())
    nf, tn, fire = nf_b.cpu().numpy(), tn_b.cpu().numpy(), fire.cpu().numpy()
    want_all = np.full(M + B, FIRE_CANARY, np.int32)           # positions >= n_fires, and the whole row of the empty utterance, keep the canary
    tail_fired, tail_silent, exact_hits, fired = 0, 0, 0, 0
    for b, T in enumerate(LENS):
        if T == 0:
            assert nf[b] == 0 and tn[b] == 0
            continue
        r = row_off[b]
        want, want_tn, exact = scan_fires(alphas[r:r + T], T, THR, TAIL)
        assert nf[b] == len(want) and tn[b] == want_tn, (b, nf[b], len(want), tn[b], want_tn)
        want_all[r + b:r + b + len(want)] = want
        assert list(fire[r + b:r + b + nf[b]]) == want, (b, list(fire[r + b:r + b + nf[b]]), want)
        tail_fired += int(bool(want) and want[-1] == T)
        tail_silent += int(not want or want[-1] != T)
        exact_hits += exact
        fired += len(want)
    assert np.array_equal(fire, want_all)
    print(f"cif_fires D={D}: {fired} fires, tail slot fired in {tail_fired} utterances and not in {tail_silent}, "
          f"alpha + integrate == threshold met {exact_hits} times")
    assert tail_fired >= 1 and tail_silent >= 1
    assert exact_hits >= 2 and fired >= 10


def test_cif_fires_offline_refusals_before_launch(ops, pkg):
    z = torch.zeros((4, 1028), dtype=torch.float32, device="cuda")
    off = torch.zeros(1, dtype=torch.int32, device="cuda")
    ln = torch.full((1,), 4, dtype=torch.int32, device="cuda")
    lib = ops._lib()
    stage = torch.zeros((5, 1028), dtype=torch.float32, device="cuda")
    cnt = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    fire = torch.full((5,), FIRE_CANARY, dtype=torch.int32, device="cuda")
    p = lambda t: t.data_ptr()
    # D > 1024, and a NULL fire_frame: hipErrorInvalidValue, nothing launched
    assert lib.pfhip_op_cif_fires(p(z), 1028, p(z), p(off), p(ln), 1, 1028, 1.0, 0.45, p(stage), p(cnt), p(cnt) + 4, p(fire), None) == 1
    assert lib.pfhip_op_cif_fires(p(z), 1028, p(z), p(off), p(ln), 1, 512, 1.0, 0.45, p(stage), p(cnt), p(cnt) + 4, None, None) == 1
    torch.cuda.synchronize()
    assert (cnt == -7).all() and (fire == FIRE_CANARY).all()
