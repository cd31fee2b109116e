"""CPU: the hotword context graph of the CTC prefix beam search (csrc/ctx_graph.cpp through pkg.ContextGraph, no device): the C
builder's dump equals the Python twin's (tests/ctc_beam_ref.py Graph) array for array, and the inputs include/pfhip.h says are
refused are refused.  Weights are multiples of 1/4, so every fp32 sum and difference of the builder is exact in both."""
import numpy as np
import pytest

import ctc_beam_ref as R

VOCAB = 50


def random_words(n, seed):
    rng = np.random.default_rng(seed)
    words = [[int(t) for t in rng.integers(1, VOCAB, size=rng.integers(2, 7))] for _ in range(n)]
    weights = [[float(x) / 4 for x in rng.integers(1, 17, size=len(w))] for w in words]
    return words, weights


CASES = {
    "none": ([], []),
    "disjoint": ([[1, 2], [3], [4, 5, 6]], [[1, 1], [2], [.5, .5, .5]]),
    "shared_prefix_equal": ([[1, 2, 3], [1, 2, 4], [1, 5]], [[1, 1, 1]] * 2 + [[1, 1]]),
    "shared_prefix_different": ([[1, 2, 3], [1, 2, 4], [1, 5]], [[3, 3, 3], [1, 1, 1], [2, 2]]),
    "prefix_of_another": ([[1, 2], [1, 2, 3], [1, 4], [7], [7, 8]], [[1, 1], [.5, .5, .5], [2, 2], [3], [1, 1]]),
    "duplicate": ([[4, 5], [4, 5], [4, 5, 6]], [[2, 2], [1, 1], [1, 1, 1]]),
    "random200": random_words(200, 5),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_dump_equals_the_python_twin(pkg, name):
    words, weights = CASES[name]
    twin = R.Graph(words, weights, VOCAB)
    g = pkg.ContextGraph(words, weights, VOCAB)
    d = g.dump()
    for key in ("arc_begin", "arc_label", "arc_next"):
        assert d[key].tolist() == getattr(twin, key).tolist(), key
    for key in ("arc_weight", "escape"):
        assert np.array_equal(d[key], getattr(twin, key)), key
    if name == "random200":
        assert len(d["escape"]) > 400 and len(d["arc_label"]) >= len(d["escape"]) - 1
    g.close()


def test_prefix_of_another_by_hand(pkg):
    """[1 2] at 1 a token inside [1 2 3] at 0.5 a token, and [1 4] at 2 a token (the derivation in csrc/ctx_graph.cpp): the node after
    1 has minCum 0.5; the node after 1 2 has minCum min(1.0, 2.0) = 1.0, is final with residual 1, carries state 0's arc (label 1,
    1 + 0.5) and keeps the escape -1, so a miss there takes the shorter word's bonus away again."""
    d = pkg.ContextGraph([[1, 2], [1, 2, 3], [1, 4]], [1.0, 0.5, 2.0], 6).dump()
    assert d["arc_begin"].tolist() == [0, 1, 3, 5]
    assert d["arc_label"].tolist() == [1, 2, 4, 1, 3] and d["arc_next"].tolist() == [1, 2, 0, 1, 0]
    assert d["arc_weight"].tolist() == [.5, .5, 3.5, 1.5, .5] and d["escape"].tolist() == [0, -.5, -1]


def test_a_scalar_weight_per_word(pkg):
    a = pkg.ContextGraph([[1, 2, 3]], [2.0], 9).dump()
    b = pkg.ContextGraph([[1, 2, 3]], [[2.0, 2.0, 2.0]], 9).dump()
    assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("words,weights,vocab", [
    ([[1, 0]], [[1, 1]], 10),                   # id 0: the escape label
    ([[1, 10]], [[1, 1]], 10),                  # id == vocab
    ([[-3]], [[1]], 10),
    ([[1], []], [[1], []], 10),                 # an empty word
    ([[1, 2]], [[1, float("inf")]], 10),
    ([[1, 2]], [[float("nan"), 1]], 10),
    ([[1, 2]], [[3e38, 3e38]], 10),             # the cumulative weight overflows fp32
    ([[1]], [[1]], 1),                          # a vocabulary without a token
])
def test_refused(pkg, words, weights, vocab):
    with pytest.raises(pkg.PfhipError) as e:
        pkg.ContextGraph(words, weights, vocab)
    assert e.value.status == 1                  # PFHIP_ERR_ARG
