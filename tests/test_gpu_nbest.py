"""GPU: N-best candidates and their log-probabilities through the C ABI (pfhip_offline_forward_nbest, pfhip_set_nbest,
pfhip_offline_fetch_nbest, pfhip_get_tensor "nbest_ids" / "nbest_logp").  An extension: the reference's GreedySearch keeps only the
arg-max (onnxruntime/src/paraformer.cpp:386-395).

Three ragged utterances, one shorter than an fbank window (n_fires = 0).  The plain model has a ragged vocabulary (1003: the head's
scalar path), the contextual one 400 (its 16-byte path)."""
import ctypes
import threading

import numpy as np
import pytest

from conftest import synth_pcm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FILL = -77          # the caller's pattern in rows the forward must not touch


def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")


def ragged(seed=31):
    rng = np.random.default_rng(seed)
    return [synth_pcm(0, 16000 * 5 + 123, rng), synth_pcm(1, 200, rng), synth_pcm(2, 16000 * 3 + 7, rng)]


@pytest.fixture(scope="module")
def plain(pkg, weights_mod):
    need_gpu()
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1)
    man, blob = weights_mod.synth_weights(cfg, seed=41)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    yield m
    m.close()


def check_candidates(r, k, logp_rows=None):
    """What every forward with candidates must satisfy; logp_rows: that call's own logp list (default r["logp"])."""
    ids, lp = r["nbest_ids"], r["nbest_logp"]
    B, max_tokens, kk = ids.shape
    assert kk == k
    logp_rows = r["logp"] if logp_rows is None else logp_rows
    for b in range(B):
        nf = int(r["n_fires"][b])
        assert (ids[b, nf:] == FILL).all() and (lp[b, nf:] == FILL).all()                     # rows >= n_fires: untouched
        n = len(r["ids"][b])
        assert np.array_equal(ids[b, :n, 0], r["ids"][b])                                     # candidate 0 is the greedy id
        assert (np.diff(lp[b, :nf], axis=1) <= 0).all()                                       # non-increasing along k
        assert ((ids[b, :nf] >= 0) & (ids[b, :nf] < r["vocab"])).all()
        if logp_rows is not None and nf:
            own = np.take_along_axis(logp_rows[b], ids[b, :nf].astype(np.int64), 1)
            assert np.array_equal(lp[b, :nf].view(np.int32), own.view(np.int32))             # bit for bit the call's own logp
            assert np.array_equal(ids[b, :nf, 0], logp_rows[b].argmax(-1))


def forward(m, utts, **kw):
    r = m.forward_ids(utts, nbest_fill=FILL, **kw)
    r["vocab"] = m.vocab_size
    return r


def test_off_is_unchanged(plain):
    utts = ragged()
    before = plain.forward_ids(utts, want_logp=True)
    forward(plain, utts, nbest=5)
    after = plain.forward_ids(utts, want_logp=True)
    assert np.array_equal(before["token_num"], after["token_num"]) and np.array_equal(before["n_fires"], after["n_fires"])
    for b in range(len(utts)):
        assert np.array_equal(before["ids"][b], after["ids"][b])
        assert np.array_equal(before["logp"][b].view(np.int32), after["logp"][b].view(np.int32))


@pytest.mark.parametrize("k", [1, 5, 8])
def test_on(plain, k):
    utts = ragged()
    off = plain.forward_ids(utts, want_logp=True)
    r = forward(plain, utts, nbest=k, want_logp=True)
    assert int(r["n_fires"][1]) == 0 and int(r["n_fires"][0]) > 0 and int(r["n_fires"][2]) > 0
    assert (r["nbest_ids"][1] == FILL).all() and (r["nbest_logp"][1] == FILL).all()           # n_fires = 0: nothing touched
    check_candidates(r, k)
    for b in range(3):                                                                        # and the rest of the result is what it was
        assert np.array_equal(r["ids"][b], off["ids"][b])
        assert np.array_equal(r["logp"][b].view(np.int32), off["logp"][b].view(np.int32))
    # without logp: the same candidates (the head forms the log-sum-exp all the same)
    q = forward(plain, utts, nbest=k)
    assert q["logp"] is None
    assert np.array_equal(q["nbest_ids"], r["nbest_ids"]) and np.array_equal(q["nbest_logp"].view(np.int32), r["nbest_logp"].view(np.int32))
    # a prefix is the answer for a smaller k
    if k > 1:
        p = forward(plain, utts, nbest=k - 1)
        assert np.array_equal(p["nbest_ids"], r["nbest_ids"][..., :k - 1])
        nf = r["n_fires"]
        for b in range(3):
            assert np.array_equal(p["nbest_logp"][b, :nf[b]].view(np.int32), r["nbest_logp"][b, :nf[b], :k - 1].view(np.int32))


def test_device_pointer_form(plain):
    utts = ragged()
    k = 4
    host = forward(plain, utts, nbest=k)
    max_tokens = host["nbest_ids"].shape[1]
    ns = np.asarray([len(u) for u in utts], np.int32)
    so = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    d_pcm = torch.from_numpy(np.concatenate(utts)).cuda()
    plain.set_nbest(k)
    try:
        plain.enqueue_device(d_pcm.data_ptr(), so, ns)
        got = plain.fetch(len(utts), max_tokens)
        nb_ids, nb_logp = plain.fetch_nbest(len(utts), max_tokens, k, fill=FILL)
        nb3_ids, _ = plain.fetch_nbest(len(utts), max_tokens, 3, fill=FILL)                   # fewer than computed: the prefix
        rows = int(got["n_fires"].sum())
        t_ids = plain.get_tensor("nbest_ids", rows * k).view(np.int32).reshape(rows, k)
        t_logp = plain.get_tensor("nbest_logp", rows * k).reshape(rows, k)
        with pytest.raises(Exception):
            plain.fetch_nbest(len(utts), max_tokens, k + 1)                                   # more than the forward computed
    finally:
        plain.set_nbest(0)
    for b in range(3):
        assert np.array_equal(got["ids"][b], host["ids"][b])
    assert np.array_equal(nb_ids, host["nbest_ids"]) and np.array_equal(nb_logp.view(np.int32), host["nbest_logp"].view(np.int32))
    assert np.array_equal(nb3_ids, host["nbest_ids"][..., :3])
    packed_ids = np.concatenate([nb_ids[b, :got["n_fires"][b]] for b in range(3)])
    packed_logp = np.concatenate([nb_logp[b, :got["n_fires"][b]] for b in range(3)])
    assert np.array_equal(t_ids, packed_ids) and np.array_equal(t_logp.view(np.int32), packed_logp.view(np.int32))
    # off again: the next enqueue computes none, and asking for them is an argument error
    plain.enqueue_device(d_pcm.data_ptr(), so, ns)
    plain.fetch(len(utts), max_tokens)
    with pytest.raises(Exception, match="status 1"):
        plain.fetch_nbest(len(utts), max_tokens, k)


def run_threads(fn, n):
    err = []

    def guard(i):
        try:
            fn(i)
        except Exception as e:          # surfaces in the main thread
            err.append(e)
    ths = [threading.Thread(target=guard, args=(i,)) for i in range(n)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    if err:
        raise err[0]


def test_merged_callers_each_get_their_own_k(pkg, weights_mod):
    """Four threads with k = 0, 1, 3, 8 under pfhip_set_batching and three contexts: a packed forward computes the largest k among
    its callers and hands each its first k.  A merged forward may tile its GEMMs differently from a lone one (test_gpu_contexts.py:
    same values to 1e-4 in the log-probabilities), so against the lone call the values are compared to that 1e-4 and the ids
    wherever the lone call's neighbouring candidates are further apart than twice that; inside each merged result the exact
    properties hold."""
    need_gpu()
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=400)
    man, blob = weights_mod.synth_weights(cfg, seed=43)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    ks = [0, 1, 3, 8]
    rng = np.random.default_rng(7)
    calls = [[synth_pcm(4 * i + j, 16000 * (2 + j) + 311 * i, rng) for j in range(2)] + [synth_pcm(9, 150, rng)] for i in range(4)]

    def one(i):
        return forward(m, calls[i], want_logp=True, **({"nbest": ks[i]} if ks[i] else {}))
    lone = [one(i) for i in range(4)]
    m.set_inflight(3)
    m.set_batching(200000, 64)
    before = m.inflight_stats()
    rounds = 3
    for _ in range(rounds):
        got = [None] * 4

        def work(i):
            got[i] = one(i)
        run_threads(work, 4)
        for i, (g, w) in enumerate(zip(got, lone)):
            assert np.array_equal(g["n_fires"], w["n_fires"]) and np.array_equal(g["token_num"], w["token_num"])
            for b in range(3):
                assert np.array_equal(g["ids"][b], w["ids"][b])
                if len(w["logp"][b]):
                    assert np.abs(g["logp"][b] - w["logp"][b]).max() < 1e-4
            if not ks[i]:
                assert "nbest_ids" not in g                                    # k = 0 in company that computes candidates: as ever
                continue
            check_candidates(g, ks[i])
            for b in range(3):
                nf = int(w["n_fires"][b])
                assert np.abs(g["nbest_logp"][b, :nf] - w["nbest_logp"][b, :nf]).max(initial=0.0) < 1e-4
                wl = w["nbest_logp"][b, :nf]
                clear = np.ones(wl.shape, bool)                               # candidates whose neighbours in the lone call are not near-ties
                gap = np.abs(np.diff(wl, axis=1)) > 2e-4
                clear[:, 1:] &= gap
                clear[:, :-1] &= gap
                # the last candidate's other neighbour (rank k + 1) is not in the list: compare it only through the values above
                clear[:, -1] = False if ks[i] > 1 else clear[:, -1]
                assert np.array_equal(g["nbest_ids"][b, :nf][clear], w["nbest_ids"][b, :nf][clear])
    after = m.inflight_stats()
    fw = sum(a["forwards"] - b["forwards"] for a, b in zip(after, before))
    n_calls = sum(a["calls"] - b["calls"] for a, b in zip(after, before))
    assert n_calls == 4 * rounds and fw < n_calls, (fw, n_calls)              # at least one packed forward served more than one call
    m.close()


def test_range_guard_rerun_produces_the_candidates_again(pkg, weights_mod):
    """pfhip_debug_poke "range_flag" (the hook of test_gpu_range_guard.py): the forward finds its flag raised and is redone on the
    exact kernels.  6 x 22 s, so that the discarded pass (in-loop split GEMMs) and the re-run (bf16 three-plane) are different
    kernels: the candidates must be the logp rows of the call -- the re-run's -- gathered at their ids."""
    need_gpu()
    cfg = weights_mod.small_config(enc_layers=3, dec_layers=1, vocab=257)
    man, blob = weights_mod.synth_weights(cfg, seed=61)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    rng = np.random.default_rng(5)
    utts = [synth_pcm(i, 16000 * 22 + 97 * i, rng) for i in range(6)]
    assert m.debug_poke("range_flag", 1) == 0
    r = forward(m, utts, nbest=5, want_logp=True)
    assert m.debug_poke("range_fallbacks") == 1
    check_candidates(r, 5)
    # one forward only: the next one is not redone, and holds the same properties on its own kernels
    r2 = forward(m, utts, nbest=5, want_logp=True)
    assert m.debug_poke("range_fallbacks") == 1
    check_candidates(r2, 5)
    m.close()


def test_contextual_model_with_two_hotword_sets(pkg, weights_mod):
    need_gpu()
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=2, vocab=400, contextual=1)
    man, blob = weights_mod.synth_weights(cfg, seed=9)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    rng = np.random.default_rng(4)
    utts = ragged(8)
    sets = [m.CompileHotwordEmbedding([list(rng.integers(2, 400, n)) for n in lens]) for lens in ((2, 3), (4, 2, 3))]
    of = [0, 1, 1]
    want = m.forward_ids(utts, want_logp=True, hw_sets=sets, set_of_utt=of)
    r = forward(m, utts, nbest=3, want_logp=True, hw_sets=sets, set_of_utt=of)
    for b in range(3):
        assert np.array_equal(r["ids"][b], want["ids"][b])
        assert np.array_equal(r["logp"][b].view(np.int32), want["logp"][b].view(np.int32))
    check_candidates(r, 3)
    one = forward(m, utts, nbest=3, hw_emb=sets[0])                           # one set for all: the hw_emb form of the wrapper
    same = m.forward_ids(utts, hw_emb=sets[0])
    for b in range(3):
        assert np.array_equal(one["ids"][b], same["ids"][b])
    check_candidates(one, 3)
    m.close()


def test_argument_errors(pkg, plain):
    utts = ragged()
    for k in (0, 9, -1):
        with pytest.raises(pkg.PfhipError, match="status 1"):
            plain.forward_ids(utts, nbest=k)
    # null buffers, straight at the C entry
    lib, B, mt = plain._lib, len(utts), 90
    bufs = [np.ascontiguousarray(u) for u in utts]
    lens = (ctypes.c_int * B)(*[len(u) for u in utts])
    ptrs = (ctypes.c_void_p * B)(*[b.ctypes.data for b in bufs])
    ids = np.zeros((B, mt), np.int32)
    tn, nf = np.zeros(B, np.int32), np.zeros(B, np.int32)
    out = pkg._Out()
    out.token_ids = ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    out.token_num = tn.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    out.n_fires = nf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    out.max_tokens = mt
    nb_ids, nb_logp = np.zeros((B, mt, 2), np.int32), np.zeros((B, mt, 2), np.float32)
    pi, pl = nb_ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), nb_logp.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    sof = (ctypes.c_int * B)(0, 0, 0)

    def call(nb):
        return lib.pfhip_offline_forward_nbest(plain._h, ptrs, lens, B, None, None, 0, sof, ctypes.byref(out),
                                               ctypes.byref(nb) if nb is not None else None)
    assert call(pkg._Nbest(2, None, pl)) == 1
    assert call(pkg._Nbest(2, pi, None)) == 1
    assert call(pkg._Nbest(2, pi, pl)) == 0
    assert call(None) == 0                                                    # nb == NULL: pfhip_offline_forward_hwsets itself
    # the device-pointer form without pfhip_set_nbest
    ns = np.asarray([len(u) for u in utts], np.int32)
    so = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    d_pcm = torch.from_numpy(np.concatenate(utts)).cuda()
    plain.enqueue_device(d_pcm.data_ptr(), so, ns)
    plain.fetch(B, mt)
    with pytest.raises(pkg.PfhipError, match="status 1"):
        plain.fetch_nbest(B, mt, 2)
    with pytest.raises(pkg.PfhipError, match="status 1"):
        plain.set_nbest(9)
