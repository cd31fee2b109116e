"""CPU: the plain-Python restatement of the CTC prefix beam search (tests/ctc_beam_ref.py) against known answers and against the sum
over all alignments.  The GPU tests of csrc/ctc_beam.hip compare with this restatement, so it is held to something independent."""
import numpy as np
import pytest

import ctc_beam_ref as R

P3 = np.array([[.5, .3, .2], [.4, .25, .35], [.6, .2, .2]])          # (blank, a, b) per frame
IDS3 = np.tile(np.arange(3), (3, 1))
A, B = 1, 2


@pytest.mark.parametrize("ft,tol", [(np.float64, 1e-12), (np.float32, 1e-6)])
def test_three_frames_known_answer(ft, tol):
    """27 alignments: [b] .284, [a] .272, [] .12 are the three best of beams 3/3."""
    r = R.search(IDS3, np.log(P3), 0, 3, 3, ft=ft, vocab=3)
    assert [h[0] for h in r["hyps"]] == [[B], [A], []]
    assert np.allclose([h[1] for h in r["hyps"]], np.log([.284, .272, .12]), atol=tol)
    assert all(h[3] == 0 and h[1] == h[2] for h in r["hyps"])


@pytest.mark.parametrize("ft,tol", [(np.float64, 1e-12), (np.float32, 1e-6)])
def test_three_frames_with_a_hotword(ft, tol):
    """Hotword [b, a] at 1 a token: [b, a] wins with ctc ln .105 and context 2; [b] loses its half match at the end (the final
    back-off) and stands at ln .244, [a] at ln .232."""
    g = R.Graph([[B, A]], [[1.0, 1.0]], 3)
    r = R.search(IDS3, np.log(P3), 0, 3, 3, graph=g, ft=ft)
    assert [h[0] for h in r["hyps"]] == [[B, A], [B], [A]]
    assert np.allclose([h[2] for h in r["hyps"]], np.log([.105, .244, .232]), atol=tol)
    assert [h[3] for h in r["hyps"]] == [2.0, 0.0, 0.0]
    assert np.allclose(r["hyps"][0][1], np.log(.105) + 2.0, atol=tol)


def test_brute_force_agrees_with_the_issue_figures():
    paths = R.all_alignments(np.log(P3))
    assert np.isclose(paths[(B,)], .284) and np.isclose(paths[(A,)], .272) and np.isclose(paths[()], .12)
    assert np.isclose(paths[(B, A)], .105) and np.isclose(sum(paths.values()), 1.0)


@pytest.mark.parametrize("T,V,seed", [(1, 2, 0), (2, 3, 1), (4, 3, 2), (5, 4, 3), (6, 3, 4), (6, 4, 5)])
def test_unpruned_search_sums_every_alignment(T, V, seed):
    """Beams wide enough that nothing is pruned (the restatement has no upper limit on them): every hypothesis's ctc score is the
    log of the sum over all its alignments."""
    rng = np.random.default_rng(seed)
    logp = np.log(rng.dirichlet(np.ones(V), size=T))
    ids = np.tile(np.arange(V), (T, 1))
    paths = R.all_alignments(logp)
    r = R.search(ids, logp, 0, V, 10 ** 6, ft=np.float64, vocab=V)
    assert r["prune_margin"] == np.inf
    got = {tuple(h[0]): h[2] for h in r["hyps"]}
    real = {k: v for k, v in got.items() if v > -R.FMAX}            # a prefix no alignment reaches keeps the "no path" score
    assert set(real) == set(paths)
    for key, p in paths.items():
        assert np.isclose(real[key], np.log(p), atol=1e-10), key


def test_merge_of_an_extension_with_a_live_hypothesis():
    """a, then b on top: [a b] arrives as extension of [a] while [a b] is already live from the frame before."""
    P = np.array([[.1, .6, .3], [.2, .2, .6], [.2, .2, .6]])
    r = R.search(np.tile(np.arange(3), (3, 1)), np.log(P), 0, 3, 16, vocab=3)
    got = {tuple(h[0]): np.exp(h[2]) for h in r["hyps"] if h[2] > -R.FMAX}
    paths = R.all_alignments(np.log(P))
    assert np.isclose(got[(A, B)], paths[(A, B)])
    assert len(got) == len(set(got))


def test_beam_one_is_the_collapse_of_the_argmax():
    rng = np.random.default_rng(11)
    logp_full = np.log(rng.dirichlet(np.ones(6) * .3, size=40))
    ids = np.argsort(-logp_full, axis=1, kind="stable")[:, :1]
    lp = np.take_along_axis(logp_full, ids, axis=1)
    r = R.search(ids, lp, 0, 1, 1, vocab=6)
    assert r["hyps"][0][0] == R.collapse(ids[:, 0].tolist())
    assert np.isclose(r["hyps"][0][1], lp.sum())


def test_empty_utterance_and_escape():
    assert R.search(np.zeros((0, 3), int), np.zeros((0, 3)), 0, 3, 3, vocab=3)["hyps"] == []
    g = R.Graph([[1, 2, 3]], [[1., 1., 1.]], 5)
    assert g.step(0, 1) == (1, 1.0) and g.step(1, 2) == (2, 1.0) and g.step(2, 3) == (0, 1.0)
    assert g.step(2, 1) == (0, -2.0)                                 # a miss is NOT tried again from state 0
    assert g.step(0, 4) == (0, 0.0)
