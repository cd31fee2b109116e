"""CPU: the numpy restatement of the hotword-biased search over a non-autoregressive head's candidates (tests/nar_beam_ref.py) against
things independent of it: the greedy sequence, a brute-force enumeration of every sequence, and seeded defects that the GPU test's
comparison must catch on the GPU test's own cases.  The GPU tests of csrc/nar_beam.hip compare with this restatement bit for bit."""
import os

import numpy as np
import pytest

import nar_beam_ref as R

F = np.float32


@pytest.fixture(scope="module")
def lib(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg.load_lib()


def dump(pkg, words, vocab=R.V):
    """The CSR arrays of the library's own builder (pfhip_ctx_graph_dump): host only."""
    return pkg.ContextGraph(words[0], words[1], vocab).dump()


def test_no_graph_hypothesis_0_is_the_greedy_sequence():
    for kind in ("random", "ties"):                                  # rows that ARE descending: column 0 is the best of each
        for (ids, lp), (w, bm, nb) in zip(R.op_utterances(kind), R.DESC):
            hyps = R.search(ids, lp, w, bm, nb)
            if len(ids) == 0:
                assert hyps == []
                continue
            assert len(hyps) == min(nb, w ** len(ids))
            assert hyps[0][0] == [min(max(int(t), 0), R.V - 1) for t in ids[:, 0]]
            am = F(0)
            for p in lp[:, 0]:
                p = F(p) if F(p) >= -R.FMAX else -R.FMAX
                with np.errstate(over="ignore"):
                    am = F(am + p)
            assert R.bits(hyps[0][2]) == R.bits(am) and R.bits(hyps[0][1]) == R.bits(am) and hyps[0][3] == 0
            for seq, *_ in hyps:
                assert len(seq) == len(ids)


def exhaustive_graphs(ids):
    """Seeded graphs over L = 4 rows of width 2: a hotword that is a proper prefix of another, one that ends on the last row, and
    one that is still unfinished at the end (its weight is taken back: the escape term)."""
    c = lambda t, j: int(ids[t, j])
    outside = next(t for t in range(1, R.V) if t not in set(ids[:, :2].ravel().tolist()))
    return {"prefix of another": ([[c(0, 1), c(1, 1)], [c(0, 1), c(1, 1), c(2, 0), c(3, 1)]], [0.7, 0.9]),
            "ends on the last row": ([[c(2, 1), c(3, 1)]], [1.3]),
            "unfinished at the end": ([[c(2, 0), c(3, 1), outside]], [1.1]),
            "all three": ([[c(0, 1), c(1, 1)], [c(0, 1), c(1, 1), c(2, 0), c(3, 1)], [c(2, 1), c(3, 1)], [c(3, 1), outside, outside]],
                          [0.7, 0.9, 1.3, 0.6])}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_exhaustive_beam_equals_brute_force(pkg, lib, seed):
    """L = 4, width 2, beam 16: all 2 ** 4 sequences stay alive, so the n best are a brute-force enumeration's, scores bit for bit.
    Brute force knows no tie rule, so the totals are first shown to be distinct."""
    ids, lp = R._rows("random", 4, 900 + seed)
    for what, words in [("no graph", None)] + list(exhaustive_graphs(ids).items()):
        g = None if words is None else dump(pkg, words)
        want = R.brute_force(ids, lp, 2, 16, graph=g)
        totals = [float(h[1]) for h in want]
        assert len(want) == 16 and len(set(totals)) == 16, f"{what}: equal totals — choose another seed"
        got = R.search(ids, lp, 2, 16, 16, graph=g)
        assert [h[0] for h in got] == [h[0] for h in want], what
        for a, b in zip(got, want):
            assert all(R.bits(x) == R.bits(y) for x, y in zip(a[1:], b[1:])), what
        if what == "unfinished at the end":      # the weight is taken back: the order is the unbiased one, and only through the escape
            assert [h[0] for h in got] == [h[0] for h in R.search(ids, lp, 2, 16, 16)] and all(h[3] == 0 for h in got)
            assert [h[0] for h in got] != [h[0] for h in R.search(ids, lp, 2, 16, 16, graph=g, defect=2)], "the escape term decides nothing"
        elif words is not None:
            assert [h[0] for h in got] != [h[0] for h in R.search(ids, lp, 2, 16, 16)], f"{what}: the graph changes nothing"


def test_dump_and_python_twin_walk_alike(pkg, lib):
    """The restatement gives the same result on the library's dump and on the Python twin of the builder (tests/ctc_beam_ref.py)."""
    import ctc_beam_ref as C
    utts = R.op_utterances("random")
    for words in R.op_words(utts):
        twin = C.Graph(words[0], [[w] * len(x) for x, w in zip(*words)], R.V)
        d = dump(pkg, words)
        for (ids, lp), (w, bm, nb) in zip(utts, R.DESC):
            a, b = R.search(ids, lp, w, bm, nb, graph=twin), R.search(ids, lp, w, bm, nb, graph=d)
            assert [h[0] for h in a] == [h[0] for h in b]
            assert all(R.bits(x[i]) == R.bits(y[i]) for x, y in zip(a, b) for i in (1, 2, 3))


def caught(pkg, defect):
    """The operator cases (kind, graph set, utterance) on which the GPU test's comparison tells the defective restatement apart."""
    hits = []
    for kind, utts, words, graph_of in R.op_cases():
        graphs = [dump(pkg, w) for w in words]
        want = R.op_reference(utts, graphs, graph_of, max(R.LENS))
        got = R.op_reference(utts, graphs, graph_of, max(R.LENS), defect=defect)
        hits += [(kind, graph_of, b) for b, (g, w) in enumerate(zip(got, want)) if R.mismatches(g, w)]
    return hits


def test_restatement_equals_itself(pkg, lib):
    assert caught(pkg, 0) == []


@pytest.mark.parametrize("defect", [1, 2, 3])
def test_seeded_defect_is_caught(pkg, lib, defect):
    """1 equal totals the other way round, 2 escape forgotten at the end, 3 candidate-major order: each changes what the GPU test
    compares on at least one of its cases (1 and 3 on the rows of dyadic values, where totals are exactly equal; 2 on the word whose
    last token never comes)."""
    hits = caught(pkg, defect)
    print(f"defect {defect}: caught on {len(hits)} (case, utterance) pairs, e.g. {hits[:3]}")
    assert hits, defect
    if defect in (1, 3):
        assert any(kind == "ties" for kind, *_ in hits)
    else:
        assert all(g != (-1, -1, -1, -1) for _, g, _ in hits)
