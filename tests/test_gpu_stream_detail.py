"""GPU: N-best candidates, confidences and fire frames per streamed token (pfhip_stream_set_detail / pfhip_stream_last_detail).

What is exact and why:
  * candidates against the GPU's own "logp" tensor of the same window: topk.hip's contract (larger value first, equal values smaller
    column first, a value is the logp entry of its column bit for bit) -- compared as bits;
  * fire frames: whether a step fires depends only on the alphas and the carried integrate, so the scalar fp32 recurrence of
    CifSearch is replayed on the GPU's own "alphas" tensors, window after window, and its steps are mapped to emitted rows by a
    row-tracking subclass of the oracle's ParaformerOnline (AddOverlapChunk's bookkeeping on indices) -- compared with ==.
Against the oracle's log-probabilities the bound is 1e-3, the BASELINE tolerance test_gpu_stream.run_both uses for "logp".
The model is test_gpu_stream's: small_config(enc_layers=3, dec_layers=2, vocab=517), one seed.
"""
import ctypes
import threading

import numpy as np
import pytest

from conftest import synth_pcm
from oracle import paraformer as P
from oracle import paraformer_online as PO

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32 = np.float32
ERR_ARG, ERR_CAPACITY = 1, 5
V = 517


@pytest.fixture(scope="module")
def small(pkg, weights_mod):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    cfg = weights_mod.small_config(enc_layers=3, dec_layers=2, vocab=V)
    man, blob = weights_mod.synth_weights(cfg, seed=77)
    model = pkg.ParaformerHip().InitAsr((man, blob))
    yield pkg, model, P.Weights(man, blob)
    model.close()


class TrackedOnline(PO.ParaformerOnline):
    """The oracle's ParaformerOnline that also knows which emitted row (0 = the first since creation / the last final call; the
    zero rows of InitCache negative) every row of feats_cache_ and of each window is a copy of.  With run_model=False ForwardChunk
    only records the window (no encoder / decoder): the front end's row counts are all that is wanted."""

    def __init__(self, W, run_model=True):
        self.run_model = run_model
        self.windows = []            # per ForwardChunk: dict(win_idx, n, is_last)
        self.rows_emitted = 0        # since creation / the last final call, updated before the reset of a final call
        super().__init__(W)

    def InitCache(self):
        super().InitCache()
        n = len(self.feats_cache_)
        self.feats_idx_ = list(range(-n, 0))
        self._new_idx, self._win_idx = [], None

    def GetPosEmb(self, wav_feats):
        self._new_idx = list(range(self.start_idx_cache_, self.start_idx_cache_ + len(wav_feats)))
        out = super().GetPosEmb(wav_feats)
        self.rows_emitted = self.start_idx_cache_
        return out

    def AddOverlapChunk(self, wav_feats, input_finished):
        new_idx = self._new_idx[len(self._new_idx) - len(wav_feats):]        # all new rows, or the last k fed again under their numbers
        idx = self.feats_idx_ + new_idx
        out = super().AddOverlapChunk(wav_feats, input_finished)
        self.feats_idx_ = idx[len(idx) - len(self.feats_cache_):]
        self._win_idx = idx + [idx[-1]] * (len(out) - len(idx))             # zero padding lies past the counted rows
        return out

    def ForwardChunk(self, chunk_feats):
        win_idx = self._win_idx if self._win_idx is not None else list(self.feats_idx_)     # (:532-540) the look-back cache alone
        self._win_idx = None
        assert len(win_idx) == len(chunk_feats)
        self.windows.append(dict(win_idx=win_idx, n=len(chunk_feats), is_last=bool(self.is_last_chunk)))
        if not self.run_model:
            return []
        return super().ForwardChunk(chunk_feats)


def replay_fires(alphas, carry, is_last, pre, suf, thr, tail):
    """CifSearch's fire decisions (paraformer-online.cpp:306-327) in scalar fp32 on one window's alphas: (steps, new carry)."""
    a = np.asarray(alphas, F32).copy()
    a[:pre] = 0
    a[suf:] = 0
    seq = [F32(carry)] + [F32(x) for x in a] + ([F32(tail)] if is_last else [])
    integ, steps = F32(0), []
    for i, alpha in enumerate(seq):
        if F32(alpha + integ) < thr:
            integ = F32(integ + alpha)
        else:
            steps.append(i)
            integ = F32(F32(integ + alpha) - thr)
    return steps, integ


def step_to_frame(step, win):
    n = win["n"]
    row = 0 if step == 0 else (step - 1 if step <= n else n - 1)
    return max(win["win_idx"][row], 0)


PLANS = {
    "six_chunks": (3, 11, [(9600, False)] * 5 + [(9600, True)]),                        # ends in a two-window final call
    "two_window_final": (6, 14, [(9600, False)] * 2 + [(14055, True)]),
    "flush_and_restart": (4, 12, [(9600, False)] * 3 + [(700, True), (9600, False), (9600, True)]),
    "one_window_final": (5, 13, [(9600, False), (9600, False), (4000, True)]),          # the tail slot of a last chunk (:557-559)
}
_records = {}


def plan_pcm(name):
    index, seed, steps = PLANS[name]
    return synth_pcm(index, sum(n for n, _ in steps), np.random.default_rng(seed)), steps


def records(small, name):
    """One stream with k = 5, fires and debug on, and the tracked oracle, over the plan -- run once, shared by the tests."""
    if name in _records:
        return _records[name]
    pkg, model, W = small
    pcm, steps = plan_pcm(name)
    on = TrackedOnline(W)
    hip = pkg.ParaformerOnlineHip(model)
    hip.set_detail(5, True)
    hip.set_debug(True)
    out, pos = [], 0
    for n, fin in steps:
        seg = pcm[pos:pos + n]
        pos += n
        w0, c0 = len(on.windows), len(on.chunk_log)
        ref_ids = on.Forward(seg, fin)
        ids = hip.Forward(seg, input_finished=fin)
        det = hip.last_detail()
        rec = dict(ids=ids, ref_ids=ref_ids, det=det, windows=on.windows[w0:], chunks=on.chunk_log[c0:], path=hip.last_path(),
                   rows_emitted=on.rows_emitted, logp=None, alphas=None)
        if rec["windows"]:
            rec["alphas"] = hip.get_tensor("alphas", 128).copy()                       # of the call's LAST window
            rec["logp"] = hip.get_tensor("logp", 128 * V).reshape(-1, V).copy()
        out.append(rec)
    hip.close()
    _records[name] = out
    return out


def top_k_of(logp_row, k):
    """Larger value first, equal values smaller column first."""
    order = sorted(range(len(logp_row)), key=lambda c: (-float(logp_row[c]), c))
    return order[:k]


@pytest.mark.parametrize("name", ["six_chunks", "flush_and_restart", "one_window_final"])
def test_candidates_and_fire_frames_exact(small, name):
    _, _, W = small
    thr, tail = F32(W.cfg["cif_threshold"]), F32(W.cfg["tail_threshold"])
    carry, checked_tokens, checked_calls, tail_fires = F32(0), 0, 0, 0
    for j, rec in enumerate(records(small, name)):
        det, ids = rec["det"], rec["ids"]
        assert det["n"] == len(ids), j
        assert list(det["ids"][:, 0]) == ids, j                                         # column 0 is the returned id
        nw = len(rec["windows"])
        if nw == 0:
            continue
        # candidates of the call's last window (all of the call where it ran one window) against the GPU's own logp
        logp = rec["logp"]
        n_last = logp.shape[0]
        assert n_last <= det["n"] and (nw == 2 or n_last == det["n"]), j
        for r in range(n_last):
            t = det["n"] - n_last + r
            want = top_k_of(logp[r], 5)
            assert list(det["ids"][t]) == want, (j, t)
            assert np.array_equal(det["logp"][t].view(np.int32), logp[r, want].view(np.int32)), (j, t)
        if nw == 1:
            win = rec["windows"][0]
            assert len(rec["alphas"]) == win["n"], j
            steps, carry = replay_fires(rec["alphas"], carry, win["is_last"], 5, 15, thr, tail)
            assert len(steps) == det["n"], (j, steps, det["n"])
            want = [step_to_frame(s, win) for s in steps]
            assert list(det["fire_frame"]) == want, (j, list(det["fire_frame"]), want)
            assert list(det["fire_ms"]) == [60 * f for f in want], j
            assert all(0 <= f < rec["rows_emitted"] for f in want), j
            tail_fires += sum(1 for s in steps if s == win["n"] + 1)
            checked_tokens += det["n"]
            checked_calls += 1
        if nw == 2 or rec["windows"][-1]["is_last"]:
            carry = F32(0)                                                              # a final call ends in Reset + InitCache
    print(f"{name}: {checked_tokens} tokens in {checked_calls} one-window calls checked exactly ({tail_fires} fired by the tail slot)")
    assert checked_tokens > 0


@pytest.mark.parametrize("name", ["six_chunks", "two_window_final", "flush_and_restart"])
def test_candidates_against_the_oracle(small, name):
    """Every call, two-window finals and the 700-sample flush included: token counts match the oracle's, every candidate's value is
    within 1e-3 of the oracle's logp at that column, and fire frames lie among the rows emitted."""
    worst, total = 0.0, 0
    paths = set()
    for j, rec in enumerate(records(small, name)):
        det = rec["det"]
        paths.add(rec["path"])
        ref_logp = [c["logp"] for c in rec["chunks"] if c["logp"] is not None]
        ref = np.concatenate(ref_logp) if ref_logp else np.zeros((0, V), F32)
        assert det["n"] == ref.shape[0] == len(rec["ref_ids"]), (j, det["n"], ref.shape)
        assert rec["ids"] == rec["ref_ids"], j
        for t in range(det["n"]):
            err = np.abs(det["logp"][t] - ref[t, det["ids"][t]])
            worst = max(worst, float(err.max()))
            assert np.all(np.diff(det["logp"][t]) <= 0), (j, t)
            assert len(set(det["ids"][t])) == 5, (j, t)
        assert all(0 <= f < rec["rows_emitted"] for f in det["fire_frame"]), (j, list(det["fire_frame"]), rec["rows_emitted"])
        if len(rec["windows"]) == 2:                       # the second window feeds rows again: its tokens come after the first's
            n1 = len(rec["chunks"][0]["ids"])
            w1, w2 = rec["windows"]
            assert all(f in [max(i, 0) for i in w1["win_idx"]] for f in det["fire_frame"][:n1]), j
            assert all(f in [max(i, 0) for i in w2["win_idx"]] for f in det["fire_frame"][n1:]), j
        total += det["n"]
    print(f"{name}: {total} tokens, worst |candidate logp - oracle logp| = {worst:.3e}, paths {sorted(paths)}")
    assert worst < 1e-3
    assert total > 0
    if name == "two_window_final":
        assert 3 in paths
    if name == "flush_and_restart":
        assert 1 in paths


def test_everything_off_changes_nothing(small):
    """k = 0 and fires off: the ids over the whole plan are those of a stream that never called the setter (and of the k = 5
    stream), and asking for candidates or fire frames is refused."""
    pkg, model, _ = small
    pcm, steps = plan_pcm("flush_and_restart")
    never, off = pkg.ParaformerOnlineHip(model), pkg.ParaformerOnlineHip(model)
    off.set_detail(0, False)
    pos = 0
    for (n, fin), rec in zip(steps, records(small, "flush_and_restart")):
        seg = pcm[pos:pos + n]
        pos += n
        a = never.Forward(seg, input_finished=fin)
        b = off.Forward(seg, input_finished=fin)
        assert a == b == rec["ids"]
        for s in (never, off):
            with pytest.raises(pkg.PfhipError) as e:
                s.last_detail(k=1, fires=False)
            assert e.value.status == ERR_ARG
            with pytest.raises(pkg.PfhipError) as e:
                s.last_detail(k=0, fires=True)
            assert e.value.status == ERR_ARG
            assert s.last_detail(k=0, fires=False)["n"] == len(a)
    never.close()
    off.close()


def run_rounds(pkg, model, waves, ks, fires):
    streams = [pkg.ParaformerOnlineHip(model) for _ in waves]
    for s, k, f in zip(streams, ks, fires):
        s.set_detail(k, f)
    plans = [[(a, min(a + 9600, len(w))) for a in range(0, len(w), 9600)] for w in waves]
    got = [[] for _ in waves]
    for j in range(max(len(p) for p in plans)):
        act = [i for i, p in enumerate(plans) if j < len(p)]
        res = pkg.ParaformerOnlineHip.forward_batch([streams[i] for i in act], [waves[i][plans[i][j][0]:plans[i][j][1]] for i in act],
                                                    [j == len(plans[i]) - 1 for i in act])
        for i, ids in zip(act, res):
            got[i].append((ids, streams[i].last_detail(), streams[i]))
    return streams, got


def test_batched_streams_keep_their_own_k(small):
    """One forward_batch plan over four streams with k = 0, 1, 5, 8 (fires on for two) and the same plan with all four at 8: each
    stream's first k are the all-8 run's prefix as bits, its ids and fire frames are identical, and a stream with fires off
    refuses fire frames."""
    pkg, model, _ = small
    rng = np.random.default_rng(8)
    waves = [synth_pcm(i, n, rng) for i, n in enumerate([9600 * 4, 9600 * 3 + 1234, 9600 * 4 + 5000, 9600 * 2 + 300])]
    ks, fires = [0, 1, 5, 8], [False, True, False, True]
    sa, mixed = run_rounds(pkg, model, waves, ks, fires)
    for i, s in enumerate(sa):                             # after each stream's last call
        if not fires[i]:
            with pytest.raises(pkg.PfhipError) as e:
                s.last_detail(k=ks[i], fires=True)
            assert e.value.status == ERR_ARG
        if ks[i] < 8:
            with pytest.raises(pkg.PfhipError) as e:
                s.last_detail(k=ks[i] + 1, fires=False)
            assert e.value.status == ERR_ARG
    sb, all8 = run_rounds(pkg, model, waves, [8] * 4, [True] * 4)
    tokens = 0
    for i in range(4):
        assert len(mixed[i]) == len(all8[i])
        for (ids_a, det_a, _), (ids_b, det_b, _) in zip(mixed[i], all8[i]):
            assert ids_a == ids_b
            assert det_a["n"] == det_b["n"] == len(ids_a)
            assert det_a["ids"].shape == (len(ids_a), ks[i])
            assert np.array_equal(det_a["ids"], det_b["ids"][:, :ks[i]])
            assert np.array_equal(det_a["logp"].view(np.int32), det_b["logp"][:, :ks[i]].view(np.int32))
            assert list(det_b["ids"][:, 0]) == ids_b
            if fires[i]:
                assert np.array_equal(det_a["fire_frame"], det_b["fire_frame"])
            else:
                assert det_a["fire_frame"] is None
            tokens += len(ids_a)
    assert tokens > 10
    for s in sa + sb:
        s.close()


def test_merged_threads_read_their_own_detail(small):
    """pfhip_set_stream_batching on, four threads with one stream each: after every call a thread's detail is its own call's -- as
    many rows as n_tokens, column 0 its ids, values descending, fire frames among the rows its stream has emitted.  Which calls
    share a forward varies from run to run, so no value is compared across runs."""
    pkg, model, W = small
    rng = np.random.default_rng(9)
    waves = [synth_pcm(20 + i, 9600 * (3 + i % 2) + 777 * i, rng) for i in range(4)]
    plans = [[(a, min(a + 9600, len(w))) for a in range(0, len(w), 9600)] for w in waves]
    emitted = []                                           # rows emitted up to each call, from the oracle's front end alone
    for w, plan in zip(waves, plans):
        on = TrackedOnline(W, run_model=False)
        rows = []
        for j, (a, b) in enumerate(plan):
            on.Forward(w[a:b], j == len(plan) - 1)
            rows.append(on.rows_emitted)
        emitted.append(rows)
    model.set_stream_batching(3000, 4)
    streams = [pkg.ParaformerOnlineHip(model) for _ in waves]
    ks = [5, 8, 1, 3]
    for s, k in zip(streams, ks):
        s.set_detail(k, True)
    problems, counts = [], [0] * 4

    def feed(i):
        try:
            for j, (a, b) in enumerate(plans[i]):
                ids = streams[i].Forward(waves[i][a:b], input_finished=(j == len(plans[i]) - 1))
                det = streams[i].last_detail()
                ok = (det["n"] == len(ids) and det["ids"].shape == (len(ids), ks[i]) and list(det["ids"][:, 0]) == ids
                      and bool(np.all(np.diff(det["logp"], axis=1) <= 0))
                      and all(0 <= f < emitted[i][j] for f in det["fire_frame"]))
                if not ok:
                    problems.append((i, j, ids, det, emitted[i][j]))
                counts[i] += len(ids)
        except Exception as e:                             # noqa: BLE001 -- reported by the main thread
            problems.append((i, repr(e)))

    ths = [threading.Thread(target=feed, args=(i,)) for i in range(4)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    model.set_stream_batching(0, 1)
    for s in streams:
        s.close()
    assert not problems, problems[:2]
    assert sum(counts) > 10


def test_refusals(small, pkg, weights_mod):
    pkg_, model, _ = small
    pcm, steps = plan_pcm("six_chunks")
    s = pkg.ParaformerOnlineHip(model)
    s.set_detail(3, True)
    for bad in (9, -1):
        with pytest.raises(pkg.PfhipError) as e:
            s.set_detail(bad, False)
        assert e.value.status == ERR_ARG
    # the refused calls left (3, True) alone: the next calls compute three candidates and fire frames
    n_tok, pos = 0, 0
    for n, fin in steps[:5]:                               # (non-final calls) up to the first one that emits a token
        ids = s.Forward(pcm[pos:pos + n], input_finished=fin)
        pos += n
        n_tok = len(ids)
        if n_tok >= 1:
            break
    assert n_tok >= 1
    det = s.last_detail(k=3, fires=True)
    assert det["n"] == n_tok and det["ids"].shape == (n_tok, 3) and list(det["ids"][:, 0]) == ids
    assert np.array_equal(s.last_detail(k=2, fires=False)["ids"], det["ids"][:, :2])      # a prefix is the answer for a smaller k
    with pytest.raises(pkg.PfhipError) as e:
        s.last_detail(k=4, fires=False)                    # more than the call computed
    assert e.value.status == ERR_ARG
    with pytest.raises(pkg.PfhipError) as e:
        s.last_detail(k=3, fires=True, cap=n_tok - 1)
    assert e.value.status == ERR_CAPACITY and e.value.n_tokens == n_tok
    assert s.last_detail(k=3, fires=True, cap=n_tok)["n"] == n_tok                        # the detail is still there
    s.Reset()
    assert s.last_detail(k=0, fires=False)["n"] == 0       # pfhip_stream_reset empties the detail
    for k, f in ((1, False), (0, True)):
        with pytest.raises(pkg.PfhipError) as e:
            s.last_detail(k=k, fires=f)
        assert e.value.status == ERR_ARG
    s.close()
    # k above the vocabulary: a model of six tokens (no forward is run on it)
    cfg = weights_mod.small_config(enc_layers=1, dec_layers=1, vocab=6)
    man, blob = weights_mod.synth_weights(cfg, seed=5)
    tiny = pkg.ParaformerHip().InitAsr((man, blob))
    t = pkg.ParaformerOnlineHip(tiny)
    t.set_detail(6, False)
    with pytest.raises(pkg.PfhipError) as e:
        t.set_detail(7, True)
    assert e.value.status == ERR_ARG
    assert t._lib.pfhip_stream_set_detail(t._h, 6, 1) == 0
    t.close()
    tiny.close()
