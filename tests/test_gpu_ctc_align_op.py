"""GPU: the Viterbi pass over the CTC trellis and the token spans (csrc/ctc_align.hip) through pfhip_op_ctc_align on given emissions.

Spans, token log-probs and score are compared BIT FOR BIT with the numpy float32 restatement (tests/ctc_align_ref.py, which
tests/test_ctc_align_ref.py holds to brute force over all paths).  The shapes are the smallest at which the kernel can go wrong: no
labels, one frame, no room for a blank, a repeated label with and without room for its blank, quantised emissions (the tie rule),
more states than the workgroup has threads (256), frame counts around 64, -inf emissions, and a ragged batch."""
import importlib

import numpy as np
import pytest

import ctc_align_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def run(ops, Es, labels, max_tokens=None):
    """One launch over the utterances (E_b, labels_b); returns per utterance (score, begin, end, logp) as numpy."""
    lab = ops.CtcLabels(labels, [E.shape[0] for E in Es])
    flat = np.concatenate([np.asarray(E, np.float32).reshape(-1) for E in Es] + [np.zeros(1, np.float32)])
    Ed = torch.from_numpy(flat).cuda()
    tb, te, tl, sc = ops.ctc_align(Ed, lab, max_tokens=max_tokens)
    torch.cuda.synchronize()
    tb, te, tl, sc = tb.cpu().numpy(), te.cpu().numpy(), tl.cpu().numpy(), sc.cpu().numpy()
    return [(sc[b], tb[b], te[b], tl[b]) for b in range(len(Es))]


def same(got, E, labels):
    score, begin, end, logp, path = ref.viterbi(E, labels)
    L = len(labels)
    g_score, g_begin, g_end, g_logp = got
    assert np.float32(g_score).tobytes() == np.float32(score).tobytes(), (g_score, score)
    assert g_begin[:L].tolist() == begin.tolist() and g_end[:L].tolist() == end.tolist()
    assert g_logp[:L].tobytes() == logp.tobytes()
    assert (g_begin[L:] == -1).all() and (g_end[L:] == -1).all()
    assert not np.isnan(g_logp).any()
    return path


def emissions(rng, N, L):
    """Log-softmax-like rows: negative, a few units wide."""
    return (-np.abs(rng.standard_normal((N, L + 1))) * 3.0).astype(np.float32)


def test_no_labels(ops):
    E = emissions(np.random.default_rng(1), 3, 0)
    (got,) = run(ops, [E], [[]])
    same(got, E, [])
    assert got[0] == np.float32(E[0, 0]) + E[1, 0] + E[2, 0]


def test_one_frame_one_label_ends_in_the_label_state(ops):
    E = np.array([[-0.1, -2.0]], np.float32)
    (got,) = run(ops, [E], [[5]])
    same(got, E, [5])
    assert got[0] == np.float32(-2.0) and got[1][0] == 0 and got[2][0] == 1


def test_as_many_frames_as_labels(ops):
    rng = np.random.default_rng(2)
    labels = [3, 4, 5, 6, 7, 8]
    E = emissions(rng, 6, 6)
    (got,) = run(ops, [E], [labels])
    same(got, E, labels)
    assert got[1][:6].tolist() == [0, 1, 2, 3, 4, 5]


def test_repeated_label(ops):
    rng = np.random.default_rng(3)
    labels = [9, 9, 4]
    E4, E3 = emissions(rng, 4, 3), emissions(rng, 3, 3)
    g4, g3 = run(ops, [E4, E3], [labels, labels])
    same(g4, E4, labels)
    assert g4[1][:3].tolist() == [0, 2, 3] and g4[2][:3].tolist() == [1, 3, 4]          # a _ a b
    same(g3, E3, labels)
    assert g3[0] == -np.inf and (g3[1] == -1).all() and (g3[2] == -1).all()


def test_tie_rule_on_quantised_emissions(ops):
    """N = 40, L = 7, emissions in {-0.5, -0.25, 0}: sums are exact, many paths tie, the rule decides.  20 seeds in one launch."""
    Es, labs = [], []
    for seed in range(20):
        rng = np.random.default_rng(100 + seed)
        labs.append([int(x) for x in rng.integers(1, 4, size=7)])
        Es.append((rng.integers(-2, 1, size=(40, 8)) * 0.25).astype(np.float32))
    for got, E, labels in zip(run(ops, Es, labs), Es, labs):
        same(got, E, labels)


@pytest.mark.parametrize("S", [255, 257, 513])
def test_more_states_than_threads(ops, S):
    L = (S - 1) // 2
    rng = np.random.default_rng(S)
    labels = [int(x) for x in rng.integers(1, 50, size=L)]
    for j in range(1, L):                                            # no equal neighbours: N = L + 3 stays feasible
        if labels[j] == labels[j - 1]:
            labels[j] = labels[j - 1] + 50
    Es = [emissions(rng, L + 3, L), emissions(rng, 2 * L, L)]
    for got, E in zip(run(ops, Es, [labels, labels]), Es):
        path = same(got, E, labels)
        assert path is not None


@pytest.mark.parametrize("N", [63, 64, 65])
def test_frame_counts_around_a_word(ops, N):
    rng = np.random.default_rng(N)
    labels = [int(x) for x in rng.integers(1, 6, size=9)]
    E = emissions(rng, N, 9)
    (got,) = run(ops, [E], [labels])
    assert same(got, E, labels) is not None


def test_minus_inf_emissions(ops):
    rng = np.random.default_rng(7)
    labels = [2, 3, 4]
    E = emissions(rng, 12, 3)
    E[:6, 2] = -np.inf                                               # label 2 cannot be emitted in the first half
    (got,) = run(ops, [E], [labels])
    same(got, E, labels)
    assert np.isfinite(got[0]) and got[1][1] >= 6
    E2 = E.copy()
    E2[:, 3] = -np.inf                                               # nowhere at all: -inf, never NaN
    (got2,) = run(ops, [E2], [labels])
    same(got2, E2, labels)
    assert got2[0] == -np.inf


def test_ragged_batch(ops):
    rng = np.random.default_rng(8)
    labs = [[1, 2, 3, 4], [], [5, 5, 5], [6, 7], [8] * 11]
    Ns = [17, 9, 4, 0, 70]                                           # utterance 2: 3 labels + 2 repeats > 4 frames; utterance 3: no frames
    Es = [emissions(rng, N, len(y)) for N, y in zip(Ns, labs)]
    got = run(ops, Es, labs, max_tokens=12)
    for g, E, y in zip(got, Es, labs):
        same(g, E, y)
    assert got[2][0] == -np.inf and got[3][0] == -np.inf
    for b in (0, 1, 4):                                              # equal to their stand-alone runs
        (alone,) = run(ops, [Es[b]], [labs[b]], max_tokens=12)
        assert alone[0].tobytes() == got[b][0].tobytes()
        for i in (1, 2, 3):
            assert alone[i].tobytes() == got[b][i].tobytes()


def test_kernel_answers_what_the_launcher_cannot_see(ops):
    """n_lab and e_off are device data: pfhip_op_ctc_align called directly (ops.ctc_align refuses the first case on the host) with an
    utterance whose n_lab exceeds max_tokens, and with one whose E_b leaves E.  Each is answered as infeasible (-inf, -1), none of
    its back-pointer bytes is written, and the utterance beside it is served as alone."""
    rng = np.random.default_rng(10)
    labs = [[1, 2, 3], [4, 5, 6, 7, 8]]
    Es = [emissions(rng, 9, 3), emissions(rng, 12, 5)]
    flat = torch.from_numpy(np.concatenate([E.reshape(-1) for E in Es])).cuda()
    lib = ops._lib()
    for case in ("n_lab above max_tokens", "E_b leaves E"):
        lab = ops.CtcLabels(labs, [9, 12])
        max_tokens = 3 if case == "n_lab above max_tokens" else 5
        if case == "E_b leaves E":
            lab.e_off = torch.tensor([0, lab.e_off_h[1] + 1], dtype=torch.int64, device="cuda")      # one float past the end
        tb = torch.full((2, max_tokens), -7, dtype=torch.int32, device="cuda")
        te, tl = tb.clone(), torch.full((2, max_tokens), float("nan"), dtype=torch.float32, device="cuda")
        sc = torch.full((2,), float("nan"), dtype=torch.float32, device="cuda")
        nbytes = ops.ctc_align_workspace_bytes(lab.e_floats)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        rc = lib.pfhip_op_ctc_align(ops._p(flat), ops._p(lab.e_off), lab.e_floats, ops._p(lab.len), ops._p(lab.n_lab), ops._p(lab.labels),
                                    ops._p(lab.lab_off), 2, max_tokens, ops._p(tb), ops._p(te), ops._p(tl), ops._p(sc), ops._p(ws), nbytes,
                                    ops._stream())
        torch.cuda.synchronize()
        assert rc == 0, case
        tb, te, tl, sc = tb.cpu().numpy(), te.cpu().numpy(), tl.cpu().numpy(), sc.cpu().numpy()
        assert sc[1] == -np.inf and (tb[1] == -1).all() and (te[1] == -1).all() and (tl[1] == -np.inf).all(), case
        same((sc[0], tb[0], te[0], tl[0]), Es[0], labs[0])
        # the back-pointer bytes of the refused utterance (from byte 2 e_off[1] on) were never written
        assert int(ws[2 * (lab.e_off_h[1] + 1):].max()) == 0, case


def test_refused_before_launch(ops, pkg):
    rng = np.random.default_rng(9)
    E = emissions(rng, 8, 3)
    lab = ops.CtcLabels([[1, 2, 3]], [8])
    Ed = torch.from_numpy(E.reshape(-1)).cuda()
    with pytest.raises(pkg.PfhipError):
        ops.ctc_align(Ed, lab, max_tokens=2)                         # fewer slots than labels
    with pytest.raises(pkg.PfhipError):
        ops.ctc_align(Ed, lab, workspace_bytes=ops.ctc_align_workspace_bytes(lab.e_floats) - 1)
    with pytest.raises(pkg.PfhipError):
        ops.ctc_align(None, lab)                                     # NULL emissions
    lib = ops._lib()
    cap = int(lib.pfhip_op_ctc_align_max_tokens())
    assert 8 * (2 * cap + 1) <= 65536 < 8 * (2 * (cap + 1) + 1)
    with pytest.raises(pkg.PfhipError):
        ops.ctc_align(Ed, lab, max_tokens=cap + 1)                   # the score rows would not fit 64 KB of LDS
    torch.cuda.synchronize()
