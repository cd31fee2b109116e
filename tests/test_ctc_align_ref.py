"""CPU: the numpy restatement of the CTC forced alignment (tests/ctc_align_ref.py) against brute force over all paths, N <= 5, L <= 3.

The GPU tests hold the kernel to the restatement bit for bit; this file holds the restatement to the definition: the optimum over
all paths, feasibility <=> N >= L + equal neighbours, L = 0, and the tie rule.  On emissions quantised to multiples of 0.25 every sum
is exact in float32, so equal scores are really equal and the rule (stay, then 1, then 2; end state 2 L preferred) picks, among the
optimal paths, the one that is largest when read from the last frame backwards."""
import numpy as np
import pytest

import ctc_align_ref as ref


def cases():
    rng = np.random.default_rng(20251020)
    out = []
    for _ in range(300):
        N = int(rng.integers(1, 6))
        L = int(rng.integers(0, 4))
        labels = [int(x) for x in rng.integers(1, 3, size=L)]        # two ids only: equal neighbours are common
        out.append((N, labels, rng))
    return out


def test_optimum_and_feasibility_against_brute_force():
    n_inf = 0
    for N, labels, rng in cases():
        E = rng.standard_normal((N, len(labels) + 1)).astype(np.float32)
        score, begin, end, logp, path = ref.viterbi(E, labels)
        best, arg = ref.brute_force(E, labels)
        assert (best > -np.inf) == ref.feasible(N, labels) == bool(score > -np.inf), (N, labels)
        if path is None:
            n_inf += 1
            assert (begin == -1).all() and (end == -1).all()
            continue
        assert tuple(int(s) for s in path) in set(ref.valid_paths(N, labels))
        assert abs(float(score) - best) <= 8 * N * np.finfo(np.float32).eps * max(1.0, np.abs(E).sum())
        assert abs(ref.path_score(E, path) - best) <= 1e-5 * max(1.0, np.abs(E).sum())
        assert ref.collapse(path, labels) == labels
        assert (ref.path_from_spans(N, begin, end) == path).all()
        for j in range(len(labels)):
            assert logp[j] == E[begin[j], j + 1]
    assert n_inf > 20          # the draw does reach infeasible cases


def test_tie_rule_on_quantised_emissions():
    n_tied = 0
    for N, labels, rng in cases():
        E = (rng.integers(-2, 1, size=(N, len(labels) + 1)) * 0.25).astype(np.float32)
        score, begin, end, logp, path = ref.viterbi(E, labels)
        best, arg = ref.brute_force(E, labels)
        if path is None:
            assert not arg
            continue
        assert float(score) == best                                  # exact sums
        n_tied += len(arg) > 1
        assert tuple(int(s) for s in path) == max(arg, key=lambda p: p[::-1])
    assert n_tied > 50


def test_no_labels():
    E = np.array([[-1.0], [-0.5], [-2.0]], np.float32)
    score, begin, end, logp, path = ref.viterbi(E, [])
    assert score == np.float32(-3.5) and len(begin) == 0 and path.tolist() == [0, 0, 0]
    assert ref.viterbi(np.zeros((0, 1), np.float32), [])[0] == 0.0
    assert ref.viterbi(np.zeros((0, 2), np.float32), [5])[0] == -np.inf


def test_repeated_label_needs_a_blank():
    labels = [7, 7, 9]
    assert not ref.feasible(3, labels) and ref.feasible(4, labels)
    E = np.zeros((4, 4), np.float32)
    score, begin, end, logp, path = ref.viterbi(E, labels)
    assert path.tolist() == [1, 2, 3, 5] and begin.tolist() == [0, 2, 3] and end.tolist() == [1, 3, 4]
    assert ref.viterbi(E[:3], labels)[0] == -np.inf


def test_minus_inf_emissions_make_no_nan():
    E = np.zeros((6, 3), np.float32)
    E[:3, 1] = -np.inf
    score, begin, end, logp, path = ref.viterbi(E, [4, 5])
    assert score == 0.0 and begin[0] >= 3
    E[:, 2] = -np.inf
    assert ref.viterbi(E, [4, 5])[0] == -np.inf
