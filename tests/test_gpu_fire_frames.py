"""GPU: fire frames of the offline CIF scan through the C ABI (pfhip_offline_forward_detail[_s16], pfhip_set_fire_frames,
pfhip_offline_fetch_fire_frames, pfhip_get_tensor "fire_frame").  An extension: the reference's only source of token times is the
timestamp head of its 4-output graph (onnxruntime/src/paraformer.cpp:545).

Three ragged utterances, one shorter than an fbank window (n_fires = 0).  The reference for the values is the CPU restatement of the
scan run on the forward's own alphas (pfhip_get_tensor "alphas"): the scan is sequential fp32, so that is exact.  Every other route a
forward can take must return the same fire frames."""
import threading

import numpy as np
import pytest

from conftest import synth_pcm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32 = np.float32
FILL = -77          # the caller's pattern in rows the forward must not touch
THR, TAIL = F32(1.0), F32(0.45)      # weights.small_config: cif_threshold, tail_threshold


def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")


def ragged(seed=31):
    rng = np.random.default_rng(seed)
    return [synth_pcm(0, 16000 * 5 + 123, rng), synth_pcm(1, 200, rng), synth_pcm(2, 16000 * 3 + 7, rng)]


def scan_fires(alphas, thr=THR, tail=TAIL):
    """cif_kernel's scalar recurrence (csrc/cif.hip), statement for statement: the loop index of every fire, T = the tail slot."""
    T = len(alphas)
    if T == 0:
        return []
    integrate, fires = F32(0.0), []
    for i in range(T + 1):
        alpha = F32(alphas[i]) if i < T else F32(tail)
        if F32(alpha + integrate) < thr:
            integrate = F32(integrate + alpha)
        else:
            fires.append(i)
            integrate = F32(integrate + alpha)
            integrate = F32(integrate - thr)
    return fires


def restated(m, r):
    """The restatement on the alphas of the forward that produced r (the model's last forward)."""
    T = [int(t) for t in r["n_frames"]]
    alphas = m.get_tensor("alphas", sum(T) + 8)
    assert len(alphas) == sum(T)
    off = np.concatenate([[0], np.cumsum(T)]).astype(int)
    return [scan_fires(alphas[off[b]:off[b + 1]]) for b in range(len(T))]


def check_fires(r, want=None):
    """What every forward with fire frames must satisfy; want: per utterance the expected list."""
    fire = r["fire_frame"]
    for b in range(fire.shape[0]):
        nf, T = int(r["n_fires"][b]), int(r["n_frames"][b])
        assert (fire[b, nf:] == FILL).all()                                 # rows >= n_fires keep the caller's fill
        assert (np.diff(fire[b, :nf]) >= 0).all() and (fire[b, :nf] >= 0).all() and (fire[b, :nf] <= T).all()
        if want is not None:
            assert list(fire[b, :nf]) == list(want[b]), (b, list(fire[b, :nf]), list(want[b]))


def forward(m, utts, **kw):
    return m.forward_ids(utts, want_fire_frames=True, fire_fill=FILL, nbest_fill=FILL, **kw)


@pytest.fixture(scope="module")
def plain(pkg, weights_mod):
    need_gpu()
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1)
    man, blob = weights_mod.synth_weights(cfg, seed=41)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    assert m.lfr_frame_ms() == 60
    yield m
    m.close()


@pytest.fixture(scope="module")
def base(plain):
    """The reference shared by the tests: the host-buffer forward with fire frames on, checked against the restatement once."""
    utts = ragged()
    r = forward(plain, utts)
    want = restated(plain, r)
    return utts, r, want


def test_fire_frames_equal_the_restatement(plain, base):
    utts, r, want = base
    assert int(r["n_fires"][1]) == 0 and int(r["n_fires"][0]) > 3 and int(r["n_fires"][2]) > 3
    assert (r["fire_frame"][1] == FILL).all()                               # n_fires = 0: its row untouched
    check_fires(r, want)
    # the inspection tensor of the same forward: [sum fires], as floats
    r2 = forward(plain, utts)
    t = plain.get_tensor("fire_frame", int(r2["n_fires"].sum()) + 4)
    assert list(t.astype(np.int64)) == [f for b in range(3) for f in want[b]]
    plain.forward_ids(utts)
    with pytest.raises(Exception, match="status 1"):
        plain.get_tensor("fire_frame", 64)                                  # a forward that recorded none has none to show


def test_off_is_unchanged(plain, base):
    utts = base[0]
    before = plain.forward_ids(utts, want_logp=True)
    with_fires = forward(plain, utts, want_logp=True)
    after = plain.forward_ids(utts, want_logp=True)
    for r in (with_fires, after):
        assert np.array_equal(before["token_num"], r["token_num"]) and np.array_equal(before["n_fires"], r["n_fires"])
        for b in range(len(utts)):
            assert np.array_equal(before["ids"][b], r["ids"][b])
            assert np.array_equal(before["logp"][b].view(np.int32), r["logp"][b].view(np.int32))
    assert "fire_frame" not in after


def test_s16_entry(plain, base):
    utts, _, want = base
    s16 = [np.round(u * 32768.0).astype(np.int16) for u in utts]           # synth_pcm makes whole 16-bit steps: exact
    assert all(np.array_equal(s.astype(F32) / F32(32768.0), u) for s, u in zip(s16, utts))
    r = forward(plain, s16)
    check_fires(r, want)


def test_with_candidates_in_the_same_call(plain, base):
    utts, r0, want = base
    nb = plain.forward_ids(utts, nbest=5, nbest_fill=FILL)
    r = forward(plain, utts, nbest=5)
    check_fires(r, want)
    assert np.array_equal(r["nbest_ids"], nb["nbest_ids"])
    assert np.array_equal(r["nbest_logp"].view(np.int32), nb["nbest_logp"].view(np.int32))
    for b in range(3):
        assert np.array_equal(r["ids"][b], r0["ids"][b])


def test_other_sample_rate_with_candidates(plain):
    """Both through one call, which pfhip_offline_forward_nbest and pfhip_offline_forward_rate each lack the form for: the result is
    that of the forward on pfhip_resample's output."""
    rng = np.random.default_rng(12)
    utts8k = [synth_pcm(0, 8000 * 4 + 11, rng), synth_pcm(2, 8000 * 2 + 5, rng)]
    rs = plain.resample(utts8k, 8000)
    want = forward(plain, rs, nbest=2)
    got = forward(plain, utts8k, nbest=2, sample_rate=8000)
    assert np.array_equal(got["n_fires"], want["n_fires"]) and int(got["n_fires"].min()) > 0
    assert np.array_equal(got["fire_frame"], want["fire_frame"])
    assert np.array_equal(got["nbest_ids"], want["nbest_ids"])
    assert np.array_equal(got["nbest_logp"].view(np.int32), want["nbest_logp"].view(np.int32))
    check_fires(got)


def test_device_pointer_forms(plain, base):
    utts, r0, want = base
    max_tokens = r0["fire_frame"].shape[1]
    ns = np.asarray([len(u) for u in utts], np.int32)
    so = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    d_pcm = torch.from_numpy(np.concatenate(utts)).cuda()
    plain.set_fire_frames(True)
    try:
        plain.enqueue_device(d_pcm.data_ptr(), so, ns)
        got = plain.fetch(len(utts), max_tokens)
        fire = plain.fetch_fire_frames(len(utts), max_tokens, fill=FILL)
        res = plain.forward_resident(d_pcm.data_ptr(), so, ns, max_tokens)
        fire_res = plain.fetch_fire_frames(len(utts), max_tokens, fill=FILL)
    finally:
        plain.set_fire_frames(False)
    for g, f in ((got, fire), (res, fire_res)):
        g["fire_frame"] = f
        for b in range(3):
            assert np.array_equal(g["ids"][b], r0["ids"][b])
        check_fires(g, want)
    # off again: the next enqueue records none, and asking for them is an argument error
    plain.enqueue_device(d_pcm.data_ptr(), so, ns)
    plain.fetch(len(utts), max_tokens)
    with pytest.raises(Exception, match="status 1"):
        plain.fetch_fire_frames(len(utts), max_tokens)


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


def test_resident_callers_sharing_one_slot_each_get_their_own(pkg, weights_mod):
    """pfhip_set_inflight(1): three threads run pfhip_offline_forward_resident with batches of 1, 2 and 3 utterances on the ONE
    execution slot of a shared handle, wait for each other, and only then call pfhip_offline_fetch_fire_frames — by then the slot
    holds whichever forward ran last, with another batch size and another max_tokens.  Every thread must get its own call's fire
    frames, in its own layout, and nothing written past its rows.  Then the main thread runs enqueue + fetch on the handle: a
    worker's later fetch_fire_frames is still its own."""
    need_gpu()
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=400)
    man, blob = weights_mod.synth_weights(cfg, seed=43)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    m.set_inflight(1)
    rng = np.random.default_rng(23)
    calls = [[synth_pcm(5 * i + j, 16000 * (2 + j + i) + 97 * i, rng) for j in range(i + 1)] for i in range(3)]
    lone = [forward(m, c) for c in calls]
    max_tok = [w["fire_frame"].shape[1] + 3 * i for i, w in enumerate(lone)]           # three different layouts
    dev = [(torch.from_numpy(np.concatenate(c)).cuda(), np.asarray([len(u) for u in c], np.int32)) for c in calls]
    m.set_fire_frames(True)
    with pytest.raises(Exception, match="status 1"):
        m.fetch_fire_frames(1, max_tok[0])                                             # this thread has fetched nothing yet
    rounds = 4
    all_ran, rounds_done, main_fetched = threading.Barrier(3), threading.Barrier(4), threading.Barrier(4)
    got = [[None] * rounds for _ in range(3)]
    late, err = [None] * 3, []

    def work(i):
        try:
            d_pcm, ns = dev[i]
            so = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
            for k in range(rounds):
                r = m.forward_resident(d_pcm.data_ptr(), so, ns, max_tok[i])
                all_ran.wait(timeout=30)                                               # every thread's forward has used the slot
                buf = np.full((len(ns) + 1, max_tok[i]), FILL, np.int32)               # one guard row behind the caller's rows
                pkg._check(m._lib, m._lib.pfhip_offline_fetch_fire_frames(m._h, buf.ctypes.data))
                r["fire_frame"], r["guard"] = buf[:-1], buf[-1]
                got[i][k] = r
                all_ran.wait(timeout=30)
            rounds_done.wait(timeout=30)
            main_fetched.wait(timeout=30)                                              # the main thread's enqueue + fetch is done
            late[i] = m.fetch_fire_frames(len(ns), max_tok[i], fill=FILL)
        except Exception as e:          # surfaces in the main thread; nobody is left waiting
            err.append(e)
            for bar in (all_ran, rounds_done, main_fetched):
                bar.abort()
    ths = [threading.Thread(target=work, args=(i,)) for i in range(3)]
    for t in ths:
        t.start()
    mine = None
    try:
        rounds_done.wait(timeout=120)
        d_pcm, ns = dev[2]
        so = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
        m.enqueue_device(d_pcm.data_ptr(), so, ns)
        mine = m.fetch(len(ns), max_tok[2])
        mine["fire_frame"] = m.fetch_fire_frames(len(ns), max_tok[2], fill=FILL)
        main_fetched.wait(timeout=30)
    except threading.BrokenBarrierError:
        pass
    finally:
        main_fetched.abort() if mine is None else None
        for t in ths:
            t.join()
        m.set_fire_frames(False)
    if err:
        raise err[0]
    for i, w in enumerate(lone):
        nw = w["fire_frame"].shape[1]
        for g in got[i]:
            assert np.array_equal(g["n_fires"], w["n_fires"])
            assert np.array_equal(g["fire_frame"][:, :nw], w["fire_frame"]) and (g["fire_frame"][:, nw:] == FILL).all()
            assert (g["guard"] == FILL).all()
            check_fires(g)
        assert np.array_equal(late[i], got[i][-1]["fire_frame"])                       # not the main thread's, not another worker's
    assert np.array_equal(mine["fire_frame"][:, :lone[2]["fire_frame"].shape[1]], lone[2]["fire_frame"])
    m.close()


def test_three_contexts_from_three_threads(pkg, weights_mod):
    """pfhip_set_inflight(3), no merging: every thread's forward runs alone on a context of its own, each with its own fire-frame
    buffer, on the kernels a lone call runs on — the same fire frames exactly."""
    need_gpu()
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=400)
    man, blob = weights_mod.synth_weights(cfg, seed=43)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    rng = np.random.default_rng(17)
    calls = [[synth_pcm(3 * i + j, 16000 * (2 + j) + 211 * i, rng) for j in range(2)] + [synth_pcm(9, 150, rng)] for i in range(3)]
    lone = [forward(m, c) for c in calls]
    for w in lone:
        check_fires(w)
    m.set_inflight(3)
    for _ in range(3):
        got = [None] * 3

        def work(i):
            got[i] = forward(m, calls[i])
        run_threads(work, 3)
        for g, w in zip(got, lone):
            assert np.array_equal(g["n_fires"], w["n_fires"])
            assert np.array_equal(g["fire_frame"], w["fire_frame"])
    m.close()


def test_merged_callers_each_get_what_they_asked_for(pkg, weights_mod):
    """Four threads under pfhip_set_batching and three contexts; they ask for fire frames, fire frames + 3 candidates, 2 candidates
    alone, and nothing.  A packed forward records fire frames when any of its callers asks and hands each caller its own
    utterances' rows.  Against the lone calls: n_fires and ids are those of the lone call (as test_gpu_nbest.py has it for merged
    callers), and so are the fire frames."""
    need_gpu()
    cfg = weights_mod.small_config(enc_layers=2, dec_layers=1, vocab=400)
    man, blob = weights_mod.synth_weights(cfg, seed=43)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    rng = np.random.default_rng(7)
    calls = [[synth_pcm(4 * i + j, 16000 * (2 + j) + 311 * i, rng) for j in range(2)] + [synth_pcm(9, 150, rng)] for i in range(4)]
    asks = [dict(want_fire_frames=True), dict(want_fire_frames=True, nbest=3), dict(nbest=2), dict()]

    def one(i):
        return m.forward_ids(calls[i], fire_fill=FILL, nbest_fill=FILL, **asks[i])
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
            assert ("fire_frame" in g) == (i < 2) and ("nbest_ids" in g) == (i in (1, 2))
            if i < 2:
                check_fires(g)
                assert np.array_equal(g["fire_frame"], w["fire_frame"])
            if i in (1, 2):
                for b in range(3):
                    assert np.array_equal(g["nbest_ids"][b, :len(g["ids"][b]), 0], g["ids"][b])
                    assert (g["nbest_ids"][b, int(g["n_fires"][b]):] == FILL).all()
    after = m.inflight_stats()
    fw = sum(a["forwards"] - b["forwards"] for a, b in zip(after, before))
    n_calls = sum(a["calls"] - b["calls"] for a, b in zip(after, before))
    assert n_calls == 4 * rounds and fw < n_calls, (fw, n_calls)              # at least one packed forward served more than one call
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
    r = forward(m, utts, want_logp=True, hw_sets=sets, set_of_utt=of)
    check_fires(r, restated(m, r))
    for b in range(3):
        assert np.array_equal(r["ids"][b], want["ids"][b])
        assert np.array_equal(r["logp"][b].view(np.int32), want["logp"][b].view(np.int32))
    one = forward(m, utts, hw_emb=sets[0])                                    # one set for all: the hw_emb form of the wrapper
    check_fires(one, restated(m, one))
    same = m.forward_ids(utts, hw_emb=sets[0])
    for b in range(3):
        assert np.array_equal(one["ids"][b], same["ids"][b])
    m.close()


def test_range_guard_rerun_records_the_fire_frames_again(pkg, weights_mod):
    """pfhip_debug_poke "range_flag" (the hook of test_gpu_range_guard.py): the forward finds its flag raised and is redone on the
    exact kernels.  6 x 22 s, as test_gpu_nbest.py has it, so that the discarded pass and the re-run are different kernels: the fire
    frames must be those of the scan over the re-run's alphas, which are what the model holds afterwards."""
    need_gpu()
    cfg = weights_mod.small_config(enc_layers=3, dec_layers=1, vocab=257)
    man, blob = weights_mod.synth_weights(cfg, seed=61)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    rng = np.random.default_rng(5)
    utts = [synth_pcm(i, 16000 * 22 + 97 * i, rng) for i in range(6)]
    assert m.debug_poke("range_flag", 1) == 0
    r = forward(m, utts)
    assert m.debug_poke("range_fallbacks") == 1
    check_fires(r, restated(m, r))
    assert int(r["n_fires"].min()) > 10
    # one forward only: the next one is not redone, and holds the same property on its own kernels
    r2 = forward(m, utts)
    assert m.debug_poke("range_fallbacks") == 1
    check_fires(r2, restated(m, r2))
    m.close()


def test_argument_errors(pkg, plain, base):
    utts = base[0]
    with pytest.raises(pkg.PfhipError, match="status 1"):
        forward(plain, utts, nbest=9)
    with pytest.raises(pkg.PfhipError, match="status 5"):
        forward(plain, utts, max_tokens=2)                                    # fewer rows than the longest token sequence
    with pytest.raises(pkg.PfhipError, match="status 1"):
        pkg._check(plain._lib, plain._lib.pfhip_offline_fetch_fire_frames(plain._h, None))      # a NULL buffer
