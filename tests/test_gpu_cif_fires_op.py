"""GPU: the CIF scan that also records where each token fired (csrc/stream.hip, cif_stream_kernel<NC, true>) through
pfhip_op_cif_stream_fires.

Everything is exact.  emb, n_fire and the carry are compared bit for bit with pfhip_op_cif_stream's on the same inputs (the sibling
runs the same statements); fire_step is compared with a restatement of oracle.paraformer_online.cif_search that also records the
loop index i of every fire (0 = the carry slot, 1..n = window rows 0..n-1, n + 1 = the tail slot).  The inputs are those of
test_gpu_row_ops.test_cif_stream_chained_bit_exact: its six window shapes, four chained chunks and alphas in steps of 1/16, so that
alpha + integrate meets the threshold exactly several times.
"""
import importlib

import numpy as np
import pytest

from oracle import paraformer_online as PO
from test_gpu_row_ops import CIF_CONNS, TAIL, THR, sixteenths

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32 = np.float32
CANARY = F32(-1234.5)
STEP_CANARY = -99


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cif_search_steps(hidden, alphas, hidden_cache, alphas_cache, chunk_size, is_last_chunk, encoder_size, tail_alphas, cif_threshold):
    """oracle.paraformer_online.cif_search, statement for statement, that also returns the loop index of every fire."""
    hidden = [h for h in hidden]
    alphas = np.asarray(alphas, F32).copy()
    alphas[:chunk_size[0]] = 0.0
    alphas[chunk_size[0] + chunk_size[1]:] = 0.0
    alphas = list(alphas)
    if len(hidden_cache) > 0:
        hidden = list(hidden_cache) + hidden
        alphas = list(alphas_cache) + alphas
    if is_last_chunk:
        hidden.append(np.zeros(encoder_size, F32))
        alphas.append(tail_alphas)
    thr = cif_threshold
    integrate = F32(0.0)
    frames = np.zeros(encoder_size, F32)
    list_frame, steps = [], []
    for i in range(len(alphas)):
        alpha = F32(alphas[i])
        if F32(alpha + integrate) < thr:
            integrate = F32(integrate + alpha)
            frames = (frames + alpha * hidden[i]).astype(F32)
        else:
            frames = (frames + F32(thr - integrate) * hidden[i]).astype(F32)
            list_frame.append(frames.copy())
            steps.append(i)
            integrate = F32(integrate + alpha)
            integrate = F32(integrate - thr)
            frames = (integrate * hidden[i]).astype(F32)
    if integrate > 0.0:
        return list_frame, steps, [(frames / integrate).astype(F32)], [integrate]
    return list_frame, steps, [frames.copy()], [integrate]


def launch_pair(ops, conns, enc, alphas, carry_plain, carry_fires, emb_rows, D):
    """pfhip_op_cif_stream and pfhip_op_cif_stream_fires on the same inputs, each on its own carry buffer."""
    B = len(conns)
    row_off = np.concatenate([[0], np.cumsum([c[0] for c in conns])[:-1]]).astype(np.int32)
    args = (row_off, [c[0] for c in conns], [c[3] for c in conns], [c[1] for c in conns], [c[2] for c in conns])
    emb_a = torch.full((B, emb_rows, D), float(CANARY), dtype=torch.float32, device="cuda")
    emb_b = emb_a.clone()
    nf_a = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    nf_b = nf_a.clone()
    steps = torch.full((B, emb_rows), STEP_CANARY, dtype=torch.int32, device="cuda")
    d_enc, d_alphas = dev(enc), dev(alphas)
    ops.cif_stream(d_enc, d_alphas, *args, carry_plain, D, THR, TAIL, emb_a, nf_a)
    ops.cif_stream_fires(d_enc, d_alphas, *args, carry_fires, D, THR, TAIL, emb_b, nf_b, steps)
    return row_off, emb_a.cpu().numpy(), nf_a.cpu().numpy(), emb_b.cpu().numpy(), nf_b.cpu().numpy(), steps.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


@pytest.mark.parametrize("D", [320, 512, 516])       # 516: the <2, true> instantiation with four channels in its second slot
def test_cif_fires_chained_exact(ops, D):
    rng = np.random.default_rng(1000 + D)
    B, emb_rows = len(CIF_CONNS), 24
    carry0 = np.zeros((B, D + 1), F32)
    carry0[:, :D] = rng.standard_normal((B, D))
    carry0[:, D] = rng.integers(1, 16, B) / 16.0
    carry0[5, D] = 0.0
    state = [([carry0[b, :D].copy()], [F32(carry0[b, D])]) for b in range(B)]
    carry_plain, carry_fires = dev(carry0), dev(carry0)
    exact_hits = fired = carry_slot_fires = tail_fires = 0
    for k in range(4):
        conns = [CIF_CONNS[(b + k) % B] for b in range(B)]
        M = sum(c[0] for c in conns)
        enc = rng.standard_normal((M, D)).astype(F32)
        alphas = sixteenths(rng, M)
        row_off, emb_a, nf_a, emb_b, nf_b, steps = launch_pair(ops, conns, enc, alphas, carry_plain, carry_fires, emb_rows, D)
        # the sibling's arithmetic is the existing kernel's, bit for bit
        assert np.array_equal(nf_a, nf_b), k
        assert same_bits(emb_a, emb_b), k
        assert same_bits(carry_plain.cpu().numpy(), carry_fires.cpu().numpy()), k
        for b, (n, pre, suf, is_last) in enumerate(conns):
            r = row_off[b]
            hid = [enc[r + i] for i in range(n)]
            before = F32(state[b][1][0])
            want_frames, want_steps, h_new, a_new = cif_search_steps(hid, alphas[r:r + n], state[b][0], state[b][1], [pre, suf - pre, 0],
                                                                     bool(is_last), D, TAIL, THR)
            ref_frames, ref_h, ref_a = PO.cif_search(hid, alphas[r:r + n], state[b][0], state[b][1], [pre, suf - pre, 0], bool(is_last), D,
                                                     TAIL, THR)
            assert len(ref_frames) == len(want_frames) and all(np.array_equal(x, y) for x, y in zip(ref_frames, want_frames))
            assert np.array_equal(ref_h[0], h_new[0]) and ref_a[0] == a_new[0]          # the restatement is the oracle's recurrence
            state[b] = (h_new, a_new)
            nf = len(want_steps)
            assert nf_b[b] == nf, (k, b)
            assert list(steps[b, :nf]) == want_steps, (k, b, list(steps[b, :nf]), want_steps)
            assert np.all(steps[b, nf:] == STEP_CANARY), (k, b)                         # untouched slots keep their canary
            assert np.array_equal(emb_b[b, :nf], np.stack(want_frames) if nf else np.zeros((0, D), F32)), (k, b)
            fired += nf
            carry_slot_fires += sum(1 for s in want_steps if s == 0)
            tail_fires += sum(1 for s in want_steps if s == n + 1)
            # exact threshold hits, counted on the oracle's recurrence as test_cif_stream_chained_bit_exact does
            integ = before
            a = alphas[r:r + n].copy()
            a[:pre] = 0
            a[suf:] = 0
            for x in list(a) + ([TAIL] if is_last else []):
                s = F32(F32(x) + integ)
                exact_hits += int(s == THR)
                integ = s if s < THR else F32(s - THR)
    print(f"cif_stream_fires D={D}: {fired} fires ({carry_slot_fires} in the carry slot, {tail_fires} in the tail slot), "
          f"alpha + integrate == threshold met {exact_hits} times")
    assert exact_hits >= 4
    assert fired > 20


def test_cif_fires_overflow_counts_and_keeps_neighbours(ops):
    """emb_rows = 4 and a connection that fires 6 times: n_fire says 6, the first four steps are stored, and the neighbours' step
    rows hold nothing but their own fire."""
    D, emb_rows = 512, 4
    rng = np.random.default_rng(77)
    conns = [(20, 5, 15, 0), (20, 5, 15, 0), (20, 5, 15, 0)]
    enc = rng.standard_normal((60, D)).astype(F32)
    alphas = np.zeros(60, F32)
    alphas[5:8] = [0.5, 0.25, 0.5]                       # connection 0: one fire, in window row 6 (carry 0.25 + 0.5 + 0.25 meets the threshold)
    alphas[20 + 6:20 + 12] = 1.0                         # connection 1: six fires, one per row 6..11
    alphas[40 + 14] = 1.0                                # connection 2: one fire on the last counted row
    carry0 = np.zeros((3, D + 1), F32)
    carry0[:, :D] = rng.standard_normal((3, D))
    carry0[:, D] = [0.25, 0.0, 0.5]
    carry_plain, carry_fires = dev(carry0), dev(carry0)
    row_off, emb_a, nf_a, emb_b, nf_b, steps = launch_pair(ops, conns, enc, alphas, carry_plain, carry_fires, emb_rows, D)
    assert list(nf_b) == [1, 6, 1] and list(nf_a) == [1, 6, 1]
    assert same_bits(emb_a, emb_b) and same_bits(carry_plain.cpu().numpy(), carry_fires.cpu().numpy())
    assert list(steps[1]) == [7, 8, 9, 10]               # rows 6..9 are steps 7..10; the fires in rows 10 and 11 are counted, not stored
    assert list(steps[0]) == [7] + [STEP_CANARY] * 3
    assert list(steps[2]) == [15] + [STEP_CANARY] * 3


def test_cif_fires_refusals_before_launch(ops, pkg):
    z = torch.zeros((4, 2048), dtype=torch.float32, device="cuda")
    nf = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    emb = torch.full((1, 4, 1028), float(CANARY), dtype=torch.float32, device="cuda")
    steps = torch.full((1, 4), STEP_CANARY, dtype=torch.int32, device="cuda")
    invalid = "hip error 1$"                              # hipErrorInvalidValue
    with pytest.raises(pkg.PfhipError, match=invalid):   # D > 1024
        ops.cif_stream_fires(z, z[0], [0], [1], [0], [0], [1], z, 1028, THR, TAIL, emb, nf, steps)
    with pytest.raises(pkg.PfhipError, match=invalid):   # a NULL buffer of pfhip_op_cif_stream's
        ops.cif_stream_fires(z, None, [0], [1], [0], [0], [1], z, 512, THR, TAIL, emb, nf, steps)
    with pytest.raises(pkg.PfhipError, match=invalid):   # a negative row offset
        ops.cif_stream_fires(z, z[0], [-1], [1], [0], [0], [1], z, 512, THR, TAIL, emb, nf, steps)
    with pytest.raises(pkg.PfhipError, match=invalid):   # a NULL fire_step
        ops.cif_stream_fires(z, z[0], [0], [1], [0], [0], [1], z, 512, THR, TAIL, emb, nf, None)
    torch.cuda.synchronize()
    assert (nf == -7).all() and (emb == float(CANARY)).all() and (steps == STEP_CANARY).all()      # nothing was launched
