"""GPU: pfhip_svs_forward_beam_sets — one SenseVoice forward, every utterance searched with its own beams and hotword graph — on the
three utterances and the weight seed of tests/test_gpu_svs_beam.py (1.0 s, 0.02 s = no rows, 2.5 s; seed 1360).

The sets: utterance 0 searches 3/3 with a one-word hotword graph, the rowless utterance 1 has a 5/5/2 set, utterance 2 searches
10/10 with nbest 4 and no graph.  `out` is pfhip_svs_forward's bit for bit.  Each utterance's result is compared with the
plain-Python restatement (tests/ctc_beam_ref.py) run on the first first_beam columns of the device's OWN k best columns, read at
their stride — the largest first_beam, 10 — from row 4 of the utterance on.  The rule is that of
tests/test_gpu_ctc_prefix_beam_op.py: e = the largest float32 / float64 difference of the restatement's scores; every prune and
final margin of the float64 run at least 16 e (else the input decides nothing: choose another weight seed with the restatement on
the head's columns); the device's hypotheses are float64's in order, scores within 4 e."""
import importlib

import numpy as np
import pytest

import ctc_beam_ref as R
from conftest import synth_pcm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SECONDS = (1.0, 0.02, 2.5)
LIDS, TEXTNORMS = [4, 0, 3], [14, 15, 15]
KW = dict(lid=LIDS, textnorm=TEXTNORMS)
HOTWORD_WEIGHT = 3.0


@pytest.fixture(scope="module")
def model(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    wt = importlib.import_module("asr_2pass_amd.weights")
    m = pkg.SenseVoiceHip().InitAsr(wt.synth_svs_weights(seed=1360), device=0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def utts():
    out = []
    for i, seconds in enumerate(SECONDS):
        x = synth_pcm(30 + i, int(seconds * 16000), np.random.default_rng(900 + i))
        out.append(np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16))
    return out


@pytest.fixture(scope="module")
def hotword(pkg, model, utts):
    """(ContextGraph, its twin, its words): the runner-up of utterance 0's plain 3/3 search as a hotword at 3 a token."""
    base = model.forward(utts, beam=(3, 3), **KW)
    best = base["beam_ids"][0][0].tolist()
    runner = next(h.tolist() for h in base["beam_ids"][0][1:] if len(h) and h.tolist() != best)
    V = int(model.cfg["vocab"])
    g = pkg.ContextGraph([runner], [HOTWORD_WEIGHT], V)
    yield g, R.Graph([runner], [[HOTWORD_WEIGHT] * len(runner)], V), [runner]
    g.close()


def sets_of(hotword):
    return [(3, 3, 3, hotword[0]), (5, 5, 2, None), (10, 10, 4, None)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_out(got, plain):
    assert got["token_num"].tolist() == plain["token_num"].tolist() and got["frame_len"].tolist() == plain["frame_len"].tolist()
    for b in range(len(plain["ids"])):
        for key in ("ids", "tok_frame", "tok_logp", "frame_ids", "frame_logp"):
            assert same_bits(got[key][b], plain[key][b]), (key, b)


def same_beam(a, b):
    assert a["beam_n_hyp"].tolist() == b["beam_n_hyp"].tolist()
    for u in range(len(a["beam_ids"])):
        assert [x.tolist() for x in a["beam_ids"][u]] == [x.tolist() for x in b["beam_ids"][u]]
        for key in ("beam_score", "beam_ctc_score", "beam_ctx_score"):
            assert same_bits(a[key][u], b[key][u]), (key, u)


def check_against_restatement(model, got, sets, twins, what=""):
    """Every utterance against the restatement on its own first_beam columns of the device's rows [M][k], k = the largest first_beam."""
    V, blank = int(model.cfg["vocab"]), int(model.cfg.get("blank_id", 0))
    T = [int(x) for x in got["frame_len"]]
    M = sum(T)
    k = max(s[0] for s in sets if s is not None)
    assert model.debug_poke("svs_topk_k") == k
    ids = model.get_tensor("ctc_topk_ids", M * k).view(np.int32).reshape(M, k)
    lp = model.get_tensor("ctc_topk_logp", M * k).reshape(M, k)
    assert ids.shape[0] == M and (ids >= 0).all() and (ids < V).all() and (np.diff(lp, axis=1) <= 0).all()
    off = 0
    for b, n in enumerate(T):
        if n:
            assert ids[off:off + n, 0].tolist() == got["frame_ids"][b].tolist()
            assert same_bits(lp[off:off + n, 0], got["frame_logp"][b])
        if sets[b] is None:
            assert got["beam_n_hyp"][b] == 0
            off += n
            continue
        fb, sb, nbest, _ = sets[b]
        rows = slice(off + 4, off + n) if n else slice(0, 0)
        run = lambda ft: R.search(ids[rows, :fb], lp[rows, :fb], blank, fb, sb, graph=twins[b], ft=ft, vocab=V, nbest=nbest)
        r64, r32 = run(np.float64), run(np.float32)
        assert [h[0] for h in r64["hyps"]] == [h[0] for h in r32["hyps"]], f"{what} utterance {b}: float32 and float64 disagree"
        e = max([abs(x[i] - y[i]) for x, y in zip(r64["hyps"], r32["hyps"]) for i in (1, 2, 3)] + [0.0])
        print(f"{what} utterance {b}: rows {max(n - 4, 0)}  e {e:.3e}  prune margin {r64['prune_margin']:.3e}  final margin {r64['final_margin']:.3e}")
        assert r64["prune_margin"] >= 16 * e and r64["final_margin"] >= 16 * e, f"{what} utterance {b}: a decision closer than 16 e"
        assert got["beam_n_hyp"][b] == len(r64["hyps"])
        worst = 0.0
        for j, (toks, s, cs, cx) in enumerate(r64["hyps"]):
            assert got["beam_ids"][b][j].tolist() == toks, (what, b, j)
            worst = max(worst, abs(got["beam_score"][b][j] - s), abs(got["beam_ctc_score"][b][j] - cs), abs(got["beam_ctx_score"][b][j] - cx))
        print(f"{what} utterance {b}: device error {worst:.3e}  bound {4 * e:.3e}")
        assert worst <= 4 * e
        off += n


def test_each_utterance_on_its_own_set(model, utts, hotword):
    plain = model.forward(utts, **KW)
    sets = sets_of(hotword)
    got = model.forward(utts, beam_sets=sets, **KW)
    same_out(got, plain)
    check_against_restatement(model, got, sets, [hotword[1], None, None], what="sets")
    assert got["beam_n_hyp"].tolist() == [3, 0, 4]
    assert got["beam_ctx_score"][0][0] > 0 and (got["beam_ctx_score"][2] == 0).all()


def test_one_set_for_all_equals_the_single_form_bit_for_bit(model, utts, hotword):
    for (fb, sb, nb, g) in ((3, 3, 3, hotword[0]), (10, 10, 4, None)):
        want = model.forward(utts, beam=(fb, sb), nbest=nb, graph=g, **KW)
        got = model.forward(utts, beam_sets=[(fb, sb, nb, g)] * 3, **KW)
        same_out(got, want)
        same_beam(got, want)


def test_an_unsearched_utterance_and_none_searched(model, utts, hotword):
    plain = model.forward(utts, **KW)
    want = model.forward(utts, beam_sets=sets_of(hotword), **KW)
    got = model.forward(utts, beam_sets=[sets_of(hotword)[0], None, None], **KW)
    same_out(got, plain)
    assert got["beam_n_hyp"].tolist() == [3, 0, 0] and model.debug_poke("svs_topk_k") == 3
    assert [x.tolist() for x in got["beam_ids"][0]] == [x.tolist() for x in want["beam_ids"][0]]      # columns of k = 3 or k = 10: the same
    assert same_bits(got["beam_score"][0], want["beam_score"][0])
    none = model.forward(utts, beam_sets=[None, None, None], **KW)                                    # the greedy head, no search
    same_out(none, plain)
    assert none["beam_n_hyp"].tolist() == [0, 0, 0] and model.debug_poke("svs_topk_k") == 0


def test_s16_and_f32_agree_bit_for_bit(model, utts, hotword):
    a = model.forward(utts, beam_sets=sets_of(hotword), **KW)
    b = model.forward([u.astype(np.float32) / np.float32(32768.0) for u in utts], beam_sets=sets_of(hotword), **KW)
    same_out(a, b)
    same_beam(a, b)


def test_the_range_guard_rerun_owns_everything(model, utts, hotword):
    before = model.debug_poke("range_fallbacks")
    assert model.debug_poke("range_flag", 1) == 0
    plain = model.forward(utts, **KW)
    assert model.debug_poke("range_fallbacks") == before + 1
    assert model.debug_poke("range_flag", 1) == 0
    sets = sets_of(hotword)
    got = model.forward(utts, beam_sets=sets, **KW)
    assert model.debug_poke("range_fallbacks") == before + 2
    same_out(got, plain)
    check_against_restatement(model, got, sets, [hotword[1], None, None], what="re-run")


def test_graphs_stay_on_the_device(pkg, model, utts, hotword):
    """A graph goes up once: the next call finds it by content (another handle with the same words included).  With a bank of 0
    bytes every graph goes up with its call, and the results are the same bits."""
    model.set_graph_bank_bytes(1 << 20)                                  # an empty bank of 1 MiB
    s0 = model.graph_bank_stats()
    assert s0["bytes_capacity"] == 1 << 20 and s0["bytes_in_use"] == 0 and s0["graphs_resident"] == 0
    first = model.forward(utts, beam_sets=sets_of(hotword), **KW)
    s1 = model.graph_bank_stats()
    assert (s1["misses"] - s0["misses"], s1["hits"] - s0["hits"]) == (1, 0) and s1["graphs_resident"] == 1 and s1["bytes_in_use"] > 0
    second = model.forward(utts, beam_sets=sets_of(hotword), **KW)
    s2 = model.graph_bank_stats()
    assert (s2["misses"] - s1["misses"], s2["hits"] - s1["hits"]) == (0, 1)
    same_beam(second, first)
    again = pkg.ContextGraph(hotword[2], [HOTWORD_WEIGHT], int(model.cfg["vocab"]))      # another handle, the same content
    third = model.forward(utts, beam_sets=[(3, 3, 3, again), (5, 5, 2, None), (10, 10, 4, None)], **KW)
    s3 = model.graph_bank_stats()
    assert (s3["misses"] - s2["misses"], s3["hits"] - s2["hits"]) == (0, 1) and s3["graphs_resident"] == 1
    same_beam(third, first)
    again.close()
    model.set_graph_bank_bytes(0)
    try:
        z0 = model.graph_bank_stats()
        assert z0["bytes_capacity"] == 0 and z0["graphs_resident"] == 0
        unbanked = model.forward(utts, beam_sets=sets_of(hotword), **KW)
        z1 = model.graph_bank_stats()
        assert z1["hits"] == z0["hits"] and z1["misses"] == z0["misses"]
    finally:
        model.set_graph_bank_bytes(16 << 20)
    same_out(unbanked, first)
    same_beam(unbanked, first)


def test_capacity_carries_the_needed_lengths(pkg, model, utts, hotword):
    want = model.forward(utts, beam_sets=sets_of(hotword), **KW)
    with pytest.raises(pkg.PfhipError) as e:
        model.forward(utts, beam_sets=sets_of(hotword), beam_max_tokens=1, **KW)
    assert e.value.status == 5                   # PFHIP_ERR_CAPACITY
    assert model.last_beam_n_tokens.shape == (3, 4)
    assert model.last_beam_n_tokens[2, 0] == len(want["beam_ids"][2][0]) > 1
    assert model.last_beam_n_tokens[0, :3].tolist() == [len(h) for h in want["beam_ids"][0]] and model.last_beam_n_tokens[0, 3] == 0


def test_refused_sets(pkg, model, utts):
    V = int(model.cfg["vocab"])
    other = pkg.ContextGraph([[1, 2]], [1.0], V + 1)
    ok = (3, 3, 3, None)
    for bad in ((0, 3, 1, None), (17, 3, 1, None), (3, 0, 1, None), (3, 17, 1, None), (3, 3, 4, None), (3, 3, 0, None), (3, 3, 3, other)):
        with pytest.raises(pkg.PfhipError) as e:
            model.forward(utts, beam_sets=[ok, None, bad], **KW)
        assert e.value.status == 1, bad          # PFHIP_ERR_ARG
    other.close()
    with pytest.raises(pkg.PfhipError):
        model.forward(utts, beam_sets=[ok, ok], **KW)
