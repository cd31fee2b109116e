"""GPU: hotwords for any Paraformer through the C ABI (pfhip_offline_forward_bias[_s16]): pfhip_offline_forward_detail plus the
hotword-biased beam search over the head's candidates (csrc/nar_beam.hip).  An extension: the reference biases a Paraformer only
through the contextual checkpoint or inside its WFST search.

The smallest synthetic Paraformer of the N-best tests (plain, vocabulary 1003), three utterances of 1, 2 and 3 s.  Hypotheses are held
to the numpy restatement (tests/nar_beam_ref.py) run on the candidates THE SAME CALL returned, bit for bit."""
import ctypes
import importlib
import threading

import numpy as np
import pytest

import nar_beam_ref as R
from conftest import synth_pcm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K = 8


@pytest.fixture(scope="module")
def model(pkg, weights_mod):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    man, blob = weights_mod.synth_weights(weights_mod.small_config(enc_layers=2, dec_layers=1), seed=41)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    yield m
    m.close()


@pytest.fixture(scope="module")
def utts():
    rng = np.random.default_rng(57)
    return [synth_pcm(0, 16000 * 1 + 123, rng), synth_pcm(1, 16000 * 2 + 7, rng), synth_pcm(2, 16000 * 3 - 55, rng)]


@pytest.fixture(scope="module")
def plain(model, utts):
    """pfhip_offline_forward_detail with the same det: the call the bias call must leave unchanged."""
    return model.forward_ids(utts, nbest=K, want_fire_frames=True, nbest_fill=-77)


@pytest.fixture(scope="module")
def words(model, plain):
    """A hotword of the SECOND-best candidates of two adjacent positions of the longest utterance, each token weighted by the gap to
    the best candidate of its row (from the returned log-probabilities) plus a margin: choosing it beats the greedy pair by 2 margins."""
    ids, lp = plain["nbest_ids"][2], plain["nbest_logp"][2]
    n = len(plain["ids"][2])
    greedy = ids[:n, 0].tolist()
    for t in sorted(range(n - 1), key=lambda t: float(lp[t, 0] - lp[t, 1] + lp[t + 1, 0] - lp[t + 1, 1])):
        a, b = int(ids[t, 1]), int(ids[t + 1, 1])
        if a >= 1 and b >= 1 and not any(greedy[i:i + 2] == [a, b] for i in range(n - 1)):
            return [a, b], [float(lp[t, 0] - lp[t, 1]) + 0.25, float(lp[t + 1, 0] - lp[t + 1, 1]) + 0.25]
    pytest.fail("no usable pair of runner-up candidates: choose another seed")


SETS = ((2, 8, 3), (8, 16, 16), (4, 4, 1))       # (width, beam, nbest) of the three sets the tests use


def run(model, utts, graph, set_of=(0, 1, 2), sets=SETS, **kw):
    return model.forward_bias(utts, [s + (graph,) for s in sets], set_of=list(set_of), nbest=K, want_fire_frames=True, nbest_fill=-77, **kw)


def same_forward(a, b):
    for key in ("token_num", "n_fires", "n_frames", "nbest_ids", "fire_frame"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["nbest_logp"].view(np.int32), b["nbest_logp"].view(np.int32))
    for x, y in zip(a["ids"], b["ids"]):
        assert np.array_equal(x, y)


def same_bias(a, b):
    for key, x in a["bias"].items():
        assert x.tobytes() == b["bias"][key].tobytes(), key


def check_against_restatement(r, graph, vocab, set_of=(0, 1, 2), sets=SETS):
    """The hypotheses are the restatement's on the candidates this call returned: ids, counts and the bits of the three scores."""
    stride = max([sets[j][2] for j in set_of if j >= 0] + [1])
    mt = r["bias"]["ids"].shape[2]
    dump = graph.dump() if graph is not None else None
    for b, j in enumerate(set_of):
        rows = min(int(r["token_num"][b]), int(r["n_fires"][b]))
        hyps = [] if j < 0 else R.search(r["nbest_ids"][b, :rows], r["nbest_logp"][b, :rows], *sets[j], graph=dump, vocab=vocab)
        bad = R.mismatches(tuple(r["bias"][key][b] for key in ("n_hyp", "ids", "n_tokens", "score", "am_score", "ctx_score")),
                           R.as_outputs(hyps, stride, mt))
        assert not bad, (b, bad)
        if j >= 0:
            assert int(r["bias"]["n_hyp"][b]) == min(sets[j][2], sets[j][0] ** rows) and rows > 0


def test_out_and_det_are_the_detail_calls(model, pkg, utts, plain, words):
    g = pkg.ContextGraph([words[0]], [words[1]], model.vocab_size)
    for graph in (None, g):
        same_forward(run(model, utts, graph), plain)
    # a det that asks for fewer candidates than the search reads, and none at all: still the detail call's
    r = model.forward_bias(utts, [(8, 16, 2, g)], nbest=3, nbest_fill=-77)
    assert np.array_equal(r["nbest_ids"], plain["nbest_ids"][..., :3])
    r = model.forward_bias(utts, [(8, 16, 2, g)])
    for x, y in zip(r["ids"], plain["ids"]):
        assert np.array_equal(x, y)


def test_hypotheses_are_the_restatements(model, pkg, utts, words):
    g = pkg.ContextGraph([words[0]], [words[1]], model.vocab_size)
    for graph in (None, g):
        check_against_restatement(run(model, utts, graph), graph, model.vocab_size)


def test_a_hotword_of_runner_up_candidates_wins(model, pkg, utts, plain, words):
    V = model.vocab_size
    a, b = words[0]
    has = lambda seq: any(list(seq[i:i + 2]) == [a, b] for i in range(len(seq) - 1))
    biased = run(model, utts, pkg.ContextGraph([words[0]], [words[1]], V))
    assert has(biased["hyps"][2][0][0]) and not has(plain["ids"][2])
    assert biased["hyps"][2][0][3] > 0 and len(biased["hyps"][2][0][0]) == len(plain["ids"][2])
    for graph in (None, pkg.ContextGraph([words[0]], [0.0], V)):      # no graph, and a graph that weighs nothing: the greedy ids
        r = run(model, utts, graph)
        for u in range(3):
            assert np.array_equal(r["hyps"][u][0][0], plain["ids"][u]) and r["hyps"][u][0][3] == 0


def test_s16_sibling_is_bit_equal(model, pkg, utts, words):
    g = pkg.ContextGraph([words[0]], [words[1]], model.vocab_size)
    s16 = [np.clip(np.round(u * 32768.0), -32768, 32767).astype(np.int16) for u in utts]
    a = run(model, s16, g)
    b = run(model, [s.astype(np.float32) / np.float32(32768.0) for s in s16], g)
    same_forward(a, b)
    same_bias(a, b)


def test_batching_and_two_contexts_give_the_same(pkg, weights_mod, utts, words):
    man, blob = weights_mod.synth_weights(weights_mod.small_config(enc_layers=2, dec_layers=1), seed=41)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    try:
        g = pkg.ContextGraph([words[0]], [words[1]], m.vocab_size)
        base = run(m, utts, g)
        m.set_inflight(2)
        got = [None, None]

        def call(i):
            got[i] = run(m, utts, g)
        threads = [threading.Thread(target=call, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        m.set_batching(2000)
        got.append(run(m, utts, g))
        for r in got:
            same_forward(r, base)
            same_bias(r, base)
    finally:
        m.close()


def test_after_a_range_guard_rerun_everything_is_the_reruns(pkg, weights_mod, utts, words):
    man, blob = weights_mod.synth_weights(weights_mod.small_config(enc_layers=2, dec_layers=1), seed=41)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    try:
        g = pkg.ContextGraph([words[0]], [words[1]], m.vocab_size)
        assert m.debug_poke("range_flag", 1) == 0
        r = run(m, utts, g)
        assert m.debug_poke("range_fallbacks") == 1
        check_against_restatement(r, g, m.vocab_size)
        assert all(int(n) > 0 for n in r["bias"]["n_hyp"])
    finally:
        m.close()


def test_an_utterance_without_a_set_has_no_hypothesis(model, pkg, utts, words):
    g = pkg.ContextGraph([words[0]], [words[1]], model.vocab_size)
    full = run(model, utts, g, set_of=(0, 2, 1))
    part = run(model, utts, g, set_of=(0, -1, 1))
    same_forward(part, full)
    check_against_restatement(part, g, model.vocab_size, set_of=(0, -1, 1))
    assert int(part["bias"]["n_hyp"][1]) == 0
    for u in (0, 2):
        for key, x in part["bias"].items():
            assert x[u].tobytes() == full["bias"][key][u].tobytes(), (u, key)


def test_capacity_and_arguments(model, pkg, utts, words):
    g = pkg.ContextGraph([words[0]], [words[1]], model.vocab_size)
    with pytest.raises(pkg.PfhipError) as e:
        run(model, utts, g, bias_max_tokens=1)
    assert e.value.status == 5                                        # PFHIP_ERR_CAPACITY: counts and scores written all the same
    full = run(model, utts, g)
    for key in ("n_hyp", "n_tokens", "score", "am_score", "ctx_score"):
        assert e.value.bias[key].tobytes() == full["bias"][key].tobytes(), key
    other = pkg.ContextGraph([[1, 2]], [1.0], model.vocab_size - 1)
    for sets, set_of, graph in ((((9, 16, 1),), (0, 0, 0), g), (((0, 16, 1),), (0, 0, 0), g), (((8, 17, 1),), (0, 0, 0), g),
                                (((8, 4, 5),), (0, 0, 0), g), (((8, 4, 0),), (0, 0, 0), g), (SETS, (0, 3, 1), g), (SETS, (0, -2, 1), g),
                                (SETS, (0, 1, 2), other)):
        with pytest.raises(pkg.PfhipError) as e:
            run(model, utts, graph, set_of=set_of, sets=sets)
        assert e.value.status == 1, (sets, set_of)                    # PFHIP_ERR_ARG


def test_a_sensevoice_handle_is_unsupported(pkg, utts):
    wt = importlib.import_module("asr_2pass_amd.weights")
    sv = pkg.SenseVoiceHip().InitAsr(wt.synth_svs_weights(seed=1360), device=0)
    try:
        lib = pkg.load_lib()
        i32 = lambda n: (ctypes.c_int32 * n)()
        pcm = np.ascontiguousarray(utts[0], np.float32)
        ptrs = (ctypes.c_void_p * 1)(pcm.ctypes.data)
        n = (ctypes.c_int * 1)(len(pcm))
        ids, tn, nf, fr = i32(64), i32(1), i32(1), i32(1)
        out = pkg._Out()
        out.token_ids, out.token_num, out.n_fires, out.n_frames, out.max_tokens = ids, tn, nf, fr, 64
        opts = pkg._BiasOpts(3, 3, 1, None)
        nh, bi, nt = i32(1), i32(64), i32(1)
        bout = pkg._BiasOut(nh, bi, nt, None, None, None, 64)
        st = lib.pfhip_offline_forward_bias(sv._h, ptrs, n, 1, 0, None, None, 0, None, ctypes.byref(out), None, ctypes.byref(opts), 1, None,
                                            ctypes.byref(bout))
        assert st == 4                                                # PFHIP_ERR_UNSUPPORTED
    finally:
        sv.close()
