"""GPU: pfhip_svs_forward_beam — the SenseVoice forward with the CTC prefix beam search (and hotwords) behind its head — on the three
utterances of test_gpu_svs_forward_spans.py (1.0 s, 0.02 s = no rows, 2.5 s) with synthetic weights.

`out` is pfhip_svs_forward's bit for bit.  The search's result is compared with the plain-Python restatement (tests/ctc_beam_ref.py)
run on the device's OWN k best columns (pfhip_get_tensor "ctc_topk_ids" / "ctc_topk_logp"), which pins the wiring: rows from 4 on,
the packing, the rowless utterance.  The rule is that of tests/test_gpu_ctc_prefix_beam_op.py: e = the largest float32 / float64
difference of the restatement's scores; every prune and final margin of the float64 run at least 16 e (else the input decides
nothing — the synthetic weights would need another seed); the device's hypotheses are float64's in order, scores within 4 e."""
import ctypes
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


@pytest.fixture(scope="module")
def model(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    wt = importlib.import_module("asr_2pass_amd.weights")
    # the seed of the synthetic weights is this file's "seed chosen beforehand": with the default one (1357) the 10/10 search of the
    # 2.5 s utterance has a prune margin of 4.3 e, with 1360 every margin of every case below is above 60 e
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


def check_against_restatement(model, got, fb, sb, nbest, graph_twin=None, what=""):
    """The search on the device's own k best columns, per utterance over its speech rows."""
    V, blank = int(model.cfg["vocab"]), int(model.cfg.get("blank_id", 0))
    T = [int(x) for x in got["frame_len"]]
    M = sum(T)
    ids = model.get_tensor("ctc_topk_ids", M * fb).view(np.int32).reshape(M, fb)
    lp = model.get_tensor("ctc_topk_logp", M * fb).reshape(M, fb)
    assert ids.shape[0] == M and (ids >= 0).all() and (ids < V).all() and (np.diff(lp, axis=1) <= 0).all()
    off = 0
    for b, n in enumerate(T):
        if n:                                    # rank 0 of every row is the frame's arg-max and its log-prob, the prompt rows included
            assert ids[off:off + n, 0].tolist() == got["frame_ids"][b].tolist()
            assert same_bits(lp[off:off + n, 0], got["frame_logp"][b])
        rows = slice(off + 4, off + n) if n else slice(0, 0)
        run = lambda ft: R.search(ids[rows], lp[rows], blank, fb, sb, graph=graph_twin, ft=ft, vocab=V, nbest=nbest)
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


@pytest.mark.parametrize("s16", [True, False])
def test_out_is_the_plain_forwards_and_beam_one_is_greedy(model, utts, s16):
    din = utts if s16 else [u.astype(np.float32) / np.float32(32768.0) for u in utts]
    plain = model.forward(din, **KW)
    got = model.forward(din, beam=(1, 1), **KW)
    same_out(got, plain)
    assert got["beam_n_hyp"].tolist() == [1, 0, 1]
    for b in (0, 2):
        # beams 1/1: the collapse of the arg-max over the SPEECH rows.  In a trained model that is ids[b][4:], the four prompt rows
        # giving the four tags; with synthetic weights the prompt rows keep any number of ids (tests/test_gpu_sensevoice_align.py
        # says the same of its "greedy tokens"), so the collapse is formed here from the frame ids behind the prompt rows.
        want = R.collapse(plain["frame_ids"][b][4:].tolist(), int(model.cfg.get("blank_id", 0)))
        assert got["beam_ids"][b][0].tolist() == want
        four_tags = R.collapse(plain["frame_ids"][b][:4].tolist(), int(model.cfg.get("blank_id", 0))) == plain["ids"][b][:4].tolist() and \
            plain["frame_ids"][b][3] != plain["frame_ids"][b][4]
        print(f"utterance {b}: the prompt rows give four tags: {four_tags} (only then is ids[b][4:] the collapse of the speech rows)")
        if four_tags:
            assert want == plain["ids"][b][4:].tolist()          # ids[b][4:] exactly
        assert got["beam_ctx_score"][b][0] == 0
    assert len(got["beam_ids"][2][0]) > 8


@pytest.mark.parametrize("beams", [(3, 3), (10, 10)])
def test_search_equals_the_restatement_on_the_devices_own_columns(model, utts, beams):
    plain = model.forward(utts, **KW)
    got = model.forward(utts, beam=beams, **KW)
    same_out(got, plain)
    check_against_restatement(model, got, beams[0], beams[1], beams[1], what=f"beams {beams}")
    assert got["beam_n_hyp"][1] == 0 and got["beam_n_hyp"][2] == beams[1]


def test_s16_and_f32_agree_bit_for_bit(model, utts):
    a = model.forward(utts, beam=(5, 5), nbest=3, **KW)
    b = model.forward([u.astype(np.float32) / np.float32(32768.0) for u in utts], beam=(5, 5), nbest=3, **KW)
    same_out(a, b)
    same_beam(a, b)
    assert a["beam_n_hyp"].tolist() == [3, 0, 3]


def test_a_hotword_changes_the_best(pkg, model, utts):
    V = int(model.cfg["vocab"])
    base = model.forward(utts, beam=(3, 3), **KW)
    best = base["beam_ids"][2][0].tolist()
    runner = next(h.tolist() for h in base["beam_ids"][2][1:] if len(h) and h.tolist() != best)
    words, weights = [runner], [3.0]
    graph = pkg.ContextGraph(words, weights, V)
    got = model.forward(utts, beam=(3, 3), graph=graph, **KW)
    same_out(got, base)
    # The best changes, holds the hotword and carries its bonus: whole matches only (an open match is backed off at the end), 3 a
    # token.  It need not BE the runner-up — on these weights a hypothesis that repeats the hotword's tokens beyond it came first.
    top = got["beam_ids"][2][0].tolist()
    assert top != best
    assert any(top[i:i + len(runner)] == runner for i in range(len(top) - len(runner) + 1))
    bonus = float(got["beam_ctx_score"][2][0])
    assert bonus > 0 and bonus % (3.0 * len(runner)) == 0
    assert got["beam_score"][2][0] > base["beam_score"][2][0]
    assert got["beam_score"][2][0] == got["beam_ctc_score"][2][0] + got["beam_ctx_score"][2][0]
    # the graph as the device got it: the float64 restatement with the graph's twin on the device's own columns
    check_against_restatement(model, got, 3, 3, 3, graph_twin=R.Graph(words, [[3.0] * len(runner)], V), what="hotword")
    graph.close()


def test_batching_on_gives_the_same(model, utts):
    want = model.forward(utts, beam=(3, 3), **KW)
    model.set_batching(2000, 8)
    try:
        got = model.forward(utts, beam=(3, 3), **KW)
    finally:
        model.set_batching(0, 8)
    same_out(got, want)
    same_beam(got, want)


def test_the_range_guard_rerun_owns_everything(model, utts):
    """The range flag raised as test_gpu_svs_forward_spans.py raises it: the forward is redone once on the exact kernels; `out` is the
    plain forward's under the same poke and the search ran on the re-run's columns (the unfused head's rows)."""
    before = model.debug_poke("range_fallbacks")
    assert model.debug_poke("range_flag", 1) == 0
    plain = model.forward(utts, **KW)
    assert model.debug_poke("range_fallbacks") == before + 1
    assert model.debug_poke("range_flag", 1) == 0
    got = model.forward(utts, beam=(3, 3), **KW)
    assert model.debug_poke("range_fallbacks") == before + 2
    same_out(got, plain)
    check_against_restatement(model, got, 3, 3, 3, what="re-run")


def test_align_works_on_the_best_ids(model, utts):
    got = model.forward(utts, beam=(3, 3), **KW)
    al = model.align([h[0] if len(h) else np.zeros(0, np.int32) for h in got["beam_ids"]])
    assert np.isfinite(al["score"][[0, 2]]).all() and len(al["begin"][2]) == len(got["beam_ids"][2][0])
    assert (al["end"][2] > al["begin"][2]).all()


def test_capacity_carries_the_needed_length(pkg, model, utts):
    want = model.forward(utts, beam=(3, 3), **KW)
    with pytest.raises(pkg.PfhipError) as e:
        model.forward(utts, beam=(3, 3), beam_max_tokens=1, **KW)
    assert e.value.status == 5                   # PFHIP_ERR_CAPACITY
    assert model.last_beam_n_tokens[2, 0] == len(want["beam_ids"][2][0]) > 1


def test_refused_arguments(pkg, model, utts):
    V = int(model.cfg["vocab"])
    other = pkg.ContextGraph([[1, 2]], [1.0], V + 1)
    for kw in (dict(beam=(0, 3)), dict(beam=(17, 3)), dict(beam=(3, 0)), dict(beam=(3, 17)), dict(beam=(3, 3), nbest=4),
               dict(beam=(3, 3), nbest=0), dict(beam=(3, 3), graph=other)):
        with pytest.raises(pkg.PfhipError) as e:
            model.forward(utts, **kw, **KW)
        assert e.value.status == 1, kw           # PFHIP_ERR_ARG
    other.close()


def test_a_paraformer_handle_is_unsupported(pkg, utts):
    wt = importlib.import_module("asr_2pass_amd.weights")
    pf = pkg.ParaformerHip().InitAsr(wt.synth_weights(wt.small_config(enc_layers=1, dec_layers=1)), device=0)
    lib = pkg.load_lib()
    i32 = lambda n: (ctypes.c_int32 * n)()
    pcm = utts[0].astype(np.float32) / np.float32(32768.0)
    ptrs = (ctypes.c_void_p * 1)(pcm.ctypes.data)
    n = (ctypes.c_int * 1)(len(pcm))
    lid, tn, nh, ids, nt = i32(1), i32(1), i32(1), i32(8), i32(1)
    out = pkg._SvsOut()
    opts = pkg._SvsBeamOpts(3, 3, 1, None)
    bo = pkg._SvsBeamOut(nh, ids, nt, None, None, None, 8)
    st = lib.pfhip_svs_forward_beam(pf._h, ptrs, n, 1, lid, tn, ctypes.byref(out), ctypes.byref(opts), ctypes.byref(bo))
    getattr(pf, "close", lambda: None)()
    assert st == 4                               # PFHIP_ERR_UNSUPPORTED
