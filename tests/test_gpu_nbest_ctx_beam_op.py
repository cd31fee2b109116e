"""GPU: the hotword-biased beam search over a non-autoregressive head's candidates (csrc/nar_beam.hip) through pfhip_op_nbest_ctx_beam
on hand-made [rows][k] arrays, against the numpy restatement tests/nar_beam_ref.py (which tests/test_nar_beam_ref.py holds to brute
force, and whose comparison it shows to catch seeded defects on these very cases).

B = 4 utterances of 0, 1, 7 and 13 rows, k = 8, V = 64, (width, beam, nbest) = (1,1,1), (3,4,2), (8,16,16), (8,16,3); graphs: none,
one word, six words with shared prefixes.  Ids, n_hyp and n_tokens are EQUAL to the restatement's and the three scores equal BIT FOR
BIT: the arithmetic is single fp32 adds in a fixed order, so no tolerance applies."""
import importlib

import numpy as np
import pytest

import nar_beam_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V, K = R.V, R.K
MAXT = max(R.LENS)


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def pack(utts, pad_rows=1):
    ids = np.concatenate([x[0] for x in utts] + [np.zeros((pad_rows, K), np.int32)]).astype(np.int32)
    lp = np.concatenate([x[1] for x in utts] + [np.zeros((pad_rows, K), np.float32)]).astype(np.float32)
    lens = [len(x[0]) for x in utts]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    return (torch.from_numpy(ids).cuda(), torch.from_numpy(lp).cuda(), torch.from_numpy(offs).cuda(),
            torch.tensor(lens, dtype=torch.int32).cuda(), sum(lens))


def per_utterance(out, b):
    return tuple(t[b] for t in out)


def launch(ops, utts, graphs, graph_of, desc=R.DESC, max_tokens=MAXT, **kw):
    ids, lp, off, n, rows = pack(utts)
    kw.setdefault("rows", rows)
    out = ops.nbest_ctx_beam(ids, lp, off, n, V, [d[0] for d in desc], [d[1] for d in desc], [d[2] for d in desc], graph_of=list(graph_of),
                             graphs=graphs, max_tokens=max_tokens, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("kind", ["random", "ties", "dirty"])
def test_equal_to_the_restatement_bit_for_bit(ops, pkg, kind):
    """random: descending rows; ties: dyadic values, many totals exactly equal (the tie rule decides); dirty: a NaN, a -inf and ids
    outside 0 .. V - 1.  Each over four assignments of the graphs to the utterances."""
    n = 0
    for k, utts, words, graph_of in R.op_cases():
        if k != kind:
            continue
        graphs = [pkg.ContextGraph(w[0], w[1], V) for w in words]
        want = R.op_reference(utts, [g.dump() for g in graphs], graph_of, MAXT)
        got = launch(ops, utts, graphs, graph_of)
        assert got[1].shape == (4, 16, MAXT)
        for b in range(4):
            bad = R.mismatches(per_utterance(got, b), want[b])
            assert not bad, (kind, graph_of, b, bad, per_utterance(got, b)[0], want[b][0])
        assert got[0].tolist() == [0, 2, 16, 3]
        n += 1
    assert n == len(R.GRAPH_SETS)


def test_hotwords_change_the_result(ops, pkg):
    """The cases are not vacuous: with the six-word graph the first hypothesis of the 13-row utterance holds a hotword the greedy
    sequence lacks, and the word whose last token never comes leaves no context score behind."""
    utts = R.op_utterances("random")
    one, five = R.op_words(utts)
    graphs = [pkg.ContextGraph(w[0], w[1], V) for w in (one, five)]
    plain = launch(ops, utts, graphs, (-1, -1, -1, -1))
    biased = launch(ops, utts, graphs, (1, 1, 1, 1))
    a, b = five[0][0]
    seq = biased[1][3, 0].tolist()
    assert any(seq[i:i + 2] == [a, b] for i in range(len(seq) - 1)) and not any(plain[1][3, 0].tolist()[i:i + 2] == [a, b] for i in range(12))
    assert biased[5][3, 0] > 0 and (plain[5] == 0).all()
    assert (biased[2][:, 0] == np.asarray(R.LENS)).all()


def test_rows_outside_the_array_give_no_hypothesis(ops, pkg):
    """The kernel is told 20 rows while the last utterance would end at row 21: it has n_hyp 0 and only the fill, and its neighbours
    are what they are without it.  The tensors and the workspace are sized for all rows, so nothing leaves memory this test owns."""
    utts = R.op_utterances("random")
    words = R.op_words(utts)
    graphs = [pkg.ContextGraph(w[0], w[1], V) for w in words]
    graph_of = (-1, 0, 1, 1)
    want = R.op_reference(utts, [g.dump() for g in graphs], graph_of, MAXT)
    got = launch(ops, utts, graphs, graph_of, rows=20)
    for b in range(3):
        assert not R.mismatches(per_utterance(got, b), want[b]), b
    assert not R.mismatches(per_utterance(got, 3), R.as_outputs([], 16, MAXT))


def test_max_tokens_below_len_truncates_ids_only(ops, pkg):
    utts = R.op_utterances("random")
    words = R.op_words(utts)
    graphs = [pkg.ContextGraph(w[0], w[1], V) for w in words]
    graph_of = (-1, 0, 1, 1)
    want = R.op_reference(utts, [g.dump() for g in graphs], graph_of, 5)
    got = launch(ops, utts, graphs, graph_of, max_tokens=5)
    for b in range(4):
        assert not R.mismatches(per_utterance(got, b), want[b]), b
    assert got[2][2, 0] == 7 and got[2][3, 0] == 13 and got[1].shape[2] == 5 and (got[1][3, :3] >= 0).all()


def test_refused_before_anything_is_written(ops, pkg):
    """Every refusal of the entry: the output buffers keep what they held."""
    utts = R.op_utterances("random")
    ids, lp, off, n, rows = pack(utts)
    hs = [pkg.ContextGraph(w[0], w[1], V) for w in R.op_words(utts)]
    other = pkg.ContextGraph([[1, 2]], [1.0], V - 1)
    wd, bm, nb = ([d[i] for d in R.DESC] for i in range(3))

    def edit(seq, b, v):
        seq = list(seq); seq[b] = v
        return seq

    bad = [dict(width=edit(wd, 1, 9)), dict(width=edit(wd, 1, 0)), dict(width=edit(wd, 1, -1)), dict(beam=edit(bm, 2, 17)),
           dict(beam=edit(bm, 1, 0)), dict(nbest=edit(nb, 1, 0)), dict(nbest=edit(nb, 1, 5)), dict(graph_of=[2, -1, -1, -1]),
           dict(graph_of=[-2, -1, -1, -1]), dict(graphs=[hs[0], other]), dict(workspace_bytes=64)]
    for kw in bad:
        out = (torch.full((4,), -7, dtype=torch.int32, device="cuda"), torch.full((4, 16, MAXT), -7, dtype=torch.int32, device="cuda"),
               torch.full((4, 16), -7, dtype=torch.int32, device="cuda")) + tuple(torch.full((4, 16), 3.5, device="cuda") for _ in range(3))
        a = dict(width=wd, beam=bm, nbest=nb, graph_of=[-1, 0, 1, 1], graphs=hs)
        a.update(kw)
        with pytest.raises(pkg.PfhipError):
            ops.nbest_ctx_beam(ids, lp, off, n, V, a.pop("width"), a.pop("beam"), a.pop("nbest"), max_tokens=MAXT, out=out, rows=rows, **a)
        torch.cuda.synchronize()
        assert all((t == -7).all() for t in out[:3]) and all((t == 3.5).all() for t in out[3:]), kw
