"""GPU: the CTC prefix beam search with every utterance on its own beams and graph in ONE launch (the per-utterance form of
csrc/ctc_beam.hip) through pfhip_op_ctc_prefix_beam_multi, against the plain-Python restatement tests/ctc_beam_ref.py.

One packed launch, V = 50, k = 10, blank 0: eight utterances whose rows are the 10 best columns of a full matrix; utterance b is held to
the restatement on the first first_beam[b] columns of its rows with its own graph.  The rule of every comparison is that of
tests/test_gpu_ctc_prefix_beam_op.py: e = the float32-against-float64 distance of the restatement on the case; every prune margin and
final margin of the float64 run is at least 16 e (a failure of THAT means "choose another seed"); the device's hypotheses are
float64's, in order; its scores are within 4 e.  e, the margins and the device's error are printed."""
import functools
import importlib

import numpy as np
import pytest

import ctc_beam_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V, K = 50, 10


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def rows_of(logp_full, k):
    """The k best columns of every row of a full [T][V] log-probability matrix, best first, lower column first among equals."""
    logp_full = np.asarray(logp_full, np.float64)
    ids = np.argsort(-logp_full, axis=1, kind="stable")[:, :k]
    return ids.astype(np.int32), np.take_along_axis(logp_full, ids, axis=1).astype(np.float32)


def random_rows(T, V, k, seed, conc=0.3):
    rng = np.random.default_rng(seed)
    return rows_of(np.log(rng.dirichlet(np.ones(V) * conc, size=T) + 1e-12), k)


def random_words(n, V, seed):
    rng = np.random.default_rng(seed)
    words = [[int(t) for t in rng.integers(1, V, size=rng.integers(2, 7))] for _ in range(n)]
    return words, [float(rng.integers(1, 9)) / 4 for _ in words]


def runner_up(rows, fb, sb):
    """The second hypothesis of the plain fb / sb search on the rows' first fb columns: a one-word graph at 1.5 a token."""
    return [R.search(rows[0][:, :fb], rows[1][:, :fb], 0, fb, sb, vocab=V)["hyps"][1][0]], [1.5]


@functools.lru_cache(maxsize=None)
def launch_case():
    """(utterances [(ids, logp)], first_beam, second_beam, nbest, graph_of, graph words [(words, weights)])."""
    u = [random_rows(37, V, K, 101, .02), random_rows(40, V, K, 101, .3), random_rows(0, V, K, 0), random_rows(300, V, K, 101, .005),
         random_rows(40, V, K, 102, .3), random_rows(12, V, K, 101, 2.0), random_rows(1, V, K, 101, 1.0), random_rows(40, V, K, 102, .3)]
    fb = [1, 3, 5, 10, 3, 10, 4, 0]
    sb = [1, 3, 5, 10, 5, 16, 4, 0]
    nb = [1, 3, 5, 4, 2, 4, 4, 0]
    graphs = [runner_up(u[1], 3, 3), random_words(200, V, 9), runner_up(u[4], 3, 5)]
    return u, fb, sb, nb, [-1, 0, -1, 1, 2, -1, -1, -1], graphs


def twin(words):
    return R.Graph(words[0], [[w] * len(x) for x, w in zip(*words)], V)


def oracle(rows, fb, sb, nb, words, ft):
    return R.search(rows[0][:, :fb], rows[1][:, :fb], 0, fb, sb, graph=None if words is None else twin(words), ft=ft, vocab=V, nbest=nb)


def reference(rows, fb, sb, nb, words, what):
    """(float64 result, e) of one utterance, its margins asserted."""
    r64, r32 = oracle(rows, fb, sb, nb, words, np.float64), oracle(rows, fb, sb, nb, words, np.float32)
    assert [h[0] for h in r64["hyps"]] == [h[0] for h in r32["hyps"]], f"{what}: float32 and float64 disagree — choose another seed"
    e = 0.0
    for x, y in zip(r64["hyps"], r32["hyps"]):
        assert x[2] > -1e30, f"{what}: a hypothesis without a path is among the n best — choose other inputs"
        e = max(e, max(abs(x[i] - y[i]) for i in (1, 2, 3)))
    print(f"{what}: e {e:.3e}  least prune margin {r64['prune_margin']:.3e}  least final margin {r64['final_margin']:.3e}")
    assert r64["prune_margin"] >= 16 * e and r64["final_margin"] >= 16 * e, f"{what}: a decision closer than 16 e — choose another seed"
    return r64, e


def pack(utts, k=K):
    ids = np.concatenate([x[0] for x in utts]).reshape(-1, k)
    lp = np.concatenate([x[1] for x in utts]).reshape(-1, k)
    lens = [len(x[0]) for x in utts]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    pad = lambda a, dt: torch.from_numpy(np.concatenate([a, np.zeros((1, k), dt)]).astype(dt)).cuda()      # never an empty tensor
    return (pad(ids, np.int32)[:len(ids)], pad(lp, np.float32)[:len(ids)], torch.from_numpy(offs).cuda(),
            torch.tensor(lens, dtype=torch.int32).cuda(), lens)


def run(ops, pkg, utts, fb, sb, nb, graph_of, graph_words, **kw):
    ids, lp, off, n, lens = pack(utts)
    graphs = [pkg.ContextGraph(w[0], w[1], V) for w in graph_words]
    out = ops.ctc_prefix_beam_multi(ids, lp, off, n, V, fb, sb, nb, graph_of=graph_of, graphs=graphs, max_tokens=max(lens), **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def assert_empty(got, b, j0=0):
    n_hyp, ids, n_tok, score, ctc, ctx = got
    assert (n_tok[b, j0:] == 0).all() and (ids[b, j0:] == -1).all()
    assert np.isneginf(score[b, j0:]).all() and np.isneginf(ctc[b, j0:]).all() and (ctx[b, j0:] == 0).all()


def check(got, utts, fb, sb, nb, graph_of, graph_words):
    n_hyp, ids, n_tok, score, ctc, ctx = got
    assert ids.shape[1] == max([n for f, n in zip(fb, nb) if f > 0] + [1])
    for b, rows in enumerate(utts):
        if fb[b] == 0 or len(rows[0]) == 0:          # no search, or no rows: no hypothesis, and the fill behind n_hyp
            assert n_hyp[b] == 0, (b, n_hyp[b])
            assert_empty(got, b)
            continue
        r64, e = reference(rows, fb[b], sb[b], nb[b], graph_words[graph_of[b]] if graph_of[b] >= 0 else None, f"utterance {b}")
        want = r64["hyps"]
        assert n_hyp[b] == len(want), (b, n_hyp[b], len(want))
        worst = 0.0
        for j, (toks, s, cs, cx) in enumerate(want):
            assert n_tok[b, j] == len(toks), (b, j)
            assert ids[b, j, :len(toks)].tolist() == toks, (b, j)
            assert (ids[b, j, len(toks):] == -1).all()
            worst = max(worst, abs(score[b, j] - s), abs(ctc[b, j] - cs), abs(ctx[b, j] - cx))
        assert_empty(got, b, len(want))              # behind n_hyp, and from nbest[b] on
        print(f"utterance {b}: device error {worst:.3e}  bound {4 * e:.3e}")
        assert worst <= 4 * e, (b, worst, 4 * e)


def test_eight_utterances_each_on_its_own_parameters(ops, pkg):
    """Beams 1/1 to 10/16, three graphs (a one-word graph twice, 200 words once), a rowless utterance and one that does not search,
    in one launch of eight workgroups."""
    utts, fb, sb, nb, graph_of, graphs = launch_case()
    got = run(ops, pkg, utts, fb, sb, nb, graph_of, graphs)
    check(got, utts, fb, sb, nb, graph_of, graphs)
    assert got[0].tolist()[2] == 0 and got[0].tolist()[7] == 0
    assert got[0][4] == 2 and got[1].shape[1] == 5   # the stride is the rowless utterance's nbest: 5


def test_same_parameters_equal_the_single_form_bit_for_bit(ops, pkg):
    utts, *_, graphs = launch_case()
    utts = [utts[1], utts[2], utts[4], utts[5]]
    ids, lp, off, n, lens = pack(utts)
    for fb, sb, nb, words in ((3, 3, 3, None), (10, 16, 4, graphs[1]), (5, 4, 2, graphs[0])):
        g = None if words is None else pkg.ContextGraph(words[0], words[1], V)
        one = ops.ctc_prefix_beam(ids, lp, off, n, V, fb, sb, nbest=nb, max_tokens=max(lens), graph=g)
        many = ops.ctc_prefix_beam_multi(ids, lp, off, n, V, [fb] * 4, [sb] * 4, [nb] * 4, graph_of=[-1 if g is None else 0] * 4,
                                         graphs=[] if g is None else [g], max_tokens=max(lens))
        torch.cuda.synchronize()
        for a, b in zip(one, many):
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (fb, sb, nb)


def test_two_utterances_share_a_graph_index(ops, pkg):
    utts, fb, sb, nb, graph_of, graphs = launch_case()
    sel = [1, 1, 4]
    args = ([utts[i] for i in sel], [fb[i] for i in sel], [sb[i] for i in sel], [nb[i] for i in sel], [1, 1, 0], [graphs[2], graphs[0]])
    got = run(ops, pkg, *args)
    check(got, *args)
    for a in got:
        assert a[0].tobytes() == a[1].tobytes()


def test_refused_before_anything_is_written(ops, pkg):
    """Every refusal of the entry: the output buffers keep what they held."""
    utts, fb, sb, nb, graph_of, graphs = launch_case()
    ids, lp, off, n, lens = pack(utts)
    hs = [pkg.ContextGraph(w[0], w[1], V) for w in graphs]
    other = pkg.ContextGraph([[1, 2]], [1.0], V - 1)

    def edit(seq, b, v):
        seq = list(seq); seq[b] = v
        return seq

    bad = [dict(first_beam=edit(fb, 1, 11)), dict(first_beam=edit(fb, 1, -1)), dict(first_beam=edit(fb, 1, 17)),
           dict(second_beam=edit(sb, 5, 17)), dict(second_beam=edit(sb, 1, -1)), dict(nbest=edit(nb, 1, 0)), dict(nbest=edit(nb, 4, 6)),
           dict(graph_of=edit(graph_of, 0, 3)), dict(graph_of=edit(graph_of, 0, -2)), dict(graphs=[hs[0], other, hs[2]]), dict(blank=V),
           dict(workspace_bytes=64)]
    for kw in bad:
        out = (torch.full((8,), -7, dtype=torch.int32, device="cuda"), torch.full((8, 5, 300), -7, dtype=torch.int32, device="cuda"),
               torch.full((8, 5), -7, dtype=torch.int32, device="cuda")) + tuple(torch.full((8, 5), 3.5, device="cuda") for _ in range(3))
        a = dict(first_beam=fb, second_beam=sb, nbest=nb, graph_of=graph_of, graphs=hs)
        a.update(kw)
        with pytest.raises(pkg.PfhipError):
            ops.ctc_prefix_beam_multi(ids, lp, off, n, V, a.pop("first_beam"), a.pop("second_beam"), a.pop("nbest"), max_tokens=300, out=out, **a)
        torch.cuda.synchronize()
        assert all((t == -7).all() for t in out[:3]) and all((t == 3.5).all() for t in out[3:]), kw


def test_untrusted_rows_stay_inside(ops, pkg):
    """Ids outside 0 .. V - 1, NaN and infinite log-probabilities, and an utterance whose rows leave the array the kernel is told of:
    the outputs are well formed and the refused utterance has no hypothesis.  The tensors hold 80 rows and the workspace is sized for
    80 while the kernel is told 64, so the third utterance's rows 60 .. 68 lie in memory this test owns whatever the kernel does."""
    rng = np.random.default_rng(5)
    ids = rng.integers(-2 ** 31, 2 ** 31 - 1, size=(80, 4)).astype(np.int32)
    lp = rng.standard_normal((80, 4)).astype(np.float32)
    lp[::3, 0] = np.nan; lp[1::5, 1] = -np.inf; lp[2::7, 2] = np.inf
    off = torch.tensor([0, 40, 60], dtype=torch.int32).cuda()
    n = torch.tensor([40, 20, 9], dtype=torch.int32).cuda()          # the third would end at row 69 of 64
    g = pkg.ContextGraph([[3, 4], [29, 1, 2]], [1.0, 0.5], 30)
    n_hyp, out, n_tok, score, ctc, ctx = ops.ctc_prefix_beam_multi(torch.from_numpy(ids).cuda(), torch.from_numpy(lp).cuda(), off, n, 30,
                                                                   [4, 2, 4], [8, 5, 8], [8, 3, 8], graph_of=[-1, 0, 0], graphs=[g],
                                                                   max_tokens=40, rows=64)
    torch.cuda.synchronize()
    n_hyp, out, n_tok = n_hyp.cpu().numpy(), out.cpu().numpy(), n_tok.cpu().numpy()
    assert n_hyp[2] == 0 and 1 <= n_hyp[0] <= 8 and 1 <= n_hyp[1] <= 3
    assert (n_tok[1, 3:] == 0).all() and (out[1, 3:] == -1).all()
    for b, T in ((0, 40), (1, 20)):
        for j in range(n_hyp[b]):
            assert 0 <= n_tok[b, j] <= T
            assert ((out[b, j, :n_tok[b, j]] >= 0) & (out[b, j, :n_tok[b, j]] < 30)).all()


def test_head_columns_do_not_depend_on_k(ops):
    """The first three columns of a row are the same bits whether the fused head ran at k = 3 or at k = 10: what lets utterances with
    different first_beam share one head launch.  (M, V) = (130, 129), K = 512: two column tiles, the second with one valid column."""
    M, Vh, Kh = 130, 129, 512
    rng = np.random.default_rng(sum(map(ord, "b129")))
    X = rng.standard_normal((M, Kh)).astype(np.float32)
    W = (rng.standard_normal((Vh, Kh)) / np.sqrt(Kh)).astype(np.float32)
    b = (0.02 * rng.standard_normal(Vh)).astype(np.float32)
    Xd, Wd, bd = (torch.from_numpy(a).cuda() for a in (X, W, b))
    ws = ops.best_w_scale(float(np.abs(W).max()))
    *_, ids3, lp3 = ops.ctc_head_topk(Xd, Wd, bd, 3, w_scale=ws)
    *_, ids10, lp10 = ops.ctc_head_topk(Xd, Wd, bd, 10, w_scale=ws)
    torch.cuda.synchronize()
    ids3, lp3, ids10, lp10 = (t.cpu().numpy() for t in (ids3, lp3, ids10, lp10))
    assert np.array_equal(ids3, ids10[:, :3])
    assert np.array_equal(lp3.view(np.uint32), lp10[:, :3].view(np.uint32))
