"""GPU: per-utterance hotword sets in one packed forward (pfhip_offline_forward_hwsets), the per-device bank that keeps the
sets' projected K/V rows across calls, contextual callers in the merge queue and on several execution contexts.

Every websocket connection of the reference's server brings its own hotword list to each Model::Forward
(websocket-server.cpp:316-359, paraformer.cpp:515-531).  The yardstick throughout is the oracle run on ONE utterance with ITS
set: n_fires equal, log-probs within 1e-3, ids through assert_ids_match (the criteria of tests/test_gpu_hotword.py)."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

from conftest import assert_ids_match, synth_pcm
from oracle import paraformer as P

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SLAB = 128 * 2 * 512 * 4           # one bank granule: 128 rows of K | V at d = 512


def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")


class Ctx:
    """One small contextual model, its oracle weights, a pool of utterances and hotword sets, and the oracle's answers (each
    computed once, shared by the tests and never changed)."""

    def __init__(self, pkg, weights_mod):
        cfg = weights_mod.small_config(enc_layers=2, dec_layers=2, vocab=400, contextual=1)
        self.man, self.blob = weights_mod.synth_weights(cfg, seed=99)
        self.pkg = pkg
        self.model = pkg.ParaformerHip().InitAsr((self.man, self.blob))
        self.W = P.Weights(self.man, self.blob)
        rng = np.random.default_rng(31)
        self.utts = [synth_pcm(i, int(n), rng) for i, n in enumerate(rng.integers(16000 * 2, 16000 * 5, 9))]
        self.sets = {}
        self._rng = np.random.default_rng(32)
        self._ref = {}

    def hotwords(self, name, n_rows):
        """A named set of n_rows rows: n_rows - 1 hotwords and the blank row CompileHotwordEmbedding appends."""
        if name not in self.sets:
            hot = [list(self._rng.integers(2, 400, int(self._rng.integers(1, 8)))) for _ in range(n_rows - 1)]
            self.sets[name] = self.model.CompileHotwordEmbedding(hot)
            assert self.sets[name].shape == (n_rows, 512)
        return self.sets[name]

    def ref(self, u, name):
        if (u, name) not in self._ref:
            self._ref[(u, name)] = P.forward_pcm(self.utts[u], self.W, hw_emb=self.sets[name])
        return self._ref[(u, name)]

    def check(self, got, b, u, name):
        ref = self.ref(u, name)
        assert int(got["n_fires"][b]) == ref["emb"].shape[0]
        err = float(np.abs(got["logp"][b] - ref["logp"]).max())
        assert err < 1e-3, f"utterance {u} with set {name}: log-prob max abs err {err}"
        assert_ids_match(got["ids"][b], ref)


@pytest.fixture(scope="module")
def ctx(pkg, weights_mod):
    need_gpu()
    c = Ctx(pkg, weights_mod)
    yield c
    c.model.close()


def run_threads(fn, n):
    err = [None] * n

    def guard(i):
        try:
            fn(i)
        except Exception as e:
            err[i] = e
    ths = [threading.Thread(target=guard, args=(i,)) for i in range(n)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    return err


def delta(after, before):
    return {k: after[k] - before[k] for k in after}


def test_mixed_batch_matches_the_oracle_per_utterance(ctx):
    """Utterances 0..3 carry sets A, B, A, C; each equals the oracle with its own set, and utterance 0 is more than 1e-3 away
    from what set B gives it: the per-utterance routing is live, a set bound to the wrong utterance would be caught."""
    m = ctx.model
    names = ["A", "B", "A", "C"]
    A, B, C = ctx.hotwords("A", 7), ctx.hotwords("B", 4), ctx.hotwords("C", 12)
    got = m.forward_ids(ctx.utts[:4], want_logp=True, hw_sets=[A, B, C], set_of_utt=[0, 1, 0, 2])
    for b, name in enumerate(names):
        ctx.check(got, b, b, name)
    wrong = ctx.ref(0, "B")
    assert wrong["logp"].shape != got["logp"][0].shape or np.abs(got["logp"][0] - wrong["logp"]).max() > 1e-3
    # a set index outside the list, and an utterance whose set is empty
    with pytest.raises(ctx.pkg.PfhipError):
        m.forward_ids(ctx.utts[:2], hw_sets=[A], set_of_utt=[0, 1])
    with pytest.raises(ctx.pkg.PfhipError, match="hw_emb is null"):
        m.forward_ids(ctx.utts[:2], hw_sets=[A, np.zeros((0, 512), np.float32)], set_of_utt=[0, 1])


def test_mixed_batch_matches_separate_one_set_calls(ctx):
    """Same handle: the packed mixed forward against one pfhip_offline_forward per utterance with its set, within the 1e-4 that
    tests/test_gpu_forward.py::test_batch_composition_invariance states for packed versus lone forwards."""
    m = ctx.model
    sets = [ctx.hotwords(n, r) for n, r in (("A", 7), ("B", 4), ("C", 12))]
    of = [0, 1, 0, 2]
    together = m.forward_ids(ctx.utts[:4], want_logp=True, hw_sets=sets, set_of_utt=of)
    for b in range(4):
        alone = m.forward_ids([ctx.utts[b]], want_logp=True, hw_emb=sets[of[b]])
        assert list(alone["ids"][0]) == list(together["ids"][b])
        assert np.abs(alone["logp"][0] - together["logp"][b]).max() < 1e-4


def test_slab_boundaries(ctx):
    """Sets of 1 (the blank row alone), 127, 128, 129 and 301 rows in one batch, in an arena of exactly their 1 + 1 + 1 + 2 + 3
    slabs: the slabs are adjacent and the arena is full.  The projection GEMM pads its rows to the 128-row tile and the slabs
    are whole tiles, so no padding reaches the next slab's keys: every utterance still equals the oracle with its set."""
    m = ctx.model
    m.set_hotword_bank_bytes(8 * SLAB)
    rows = [1, 127, 128, 129, 301]
    names = [f"S{r}" for r in rows]
    sets = [ctx.hotwords(n, r) for n, r in zip(names, rows)]
    before = m.hotword_bank_stats()
    got = m.forward_ids(ctx.utts[:5], want_logp=True, hw_sets=sets, set_of_utt=list(range(5)))
    st = m.hotword_bank_stats()
    assert st["bytes_capacity"] == 8 * SLAB and st["bytes_in_use"] == 8 * SLAB and st["sets_resident"] == 5
    d = delta(st, before)
    assert d["misses"] == 5 and d["per_call_forwards"] == 0 and st["max_sets_in_forward"] >= 5
    for b, name in enumerate(names):
        ctx.check(got, b, b, name)
    # the same batch again, the sets in another order: all hits, same answers
    order = [4, 2, 0, 3, 1]
    again = m.forward_ids([ctx.utts[b] for b in order], want_logp=True, hw_sets=sets, set_of_utt=order)
    d = delta(m.hotword_bank_stats(), st)
    assert d["hits"] == 5 and d["misses"] == 0 and d["evictions"] == 0
    for i, b in enumerate(order):
        ctx.check(again, i, b, names[b])
        assert np.array_equal(again["logp"][i], got["logp"][b]) or np.abs(again["logp"][i] - got["logp"][b]).max() < 1e-4
    m.set_hotword_bank_bytes(64 << 20)


def test_bank_hits_misses_eviction_and_oversize_sets(ctx):
    m = ctx.model
    m.set_hotword_bank_bytes(2 * SLAB)                       # room for two one-slab sets
    A, B = ctx.hotwords("A", 7), ctx.hotwords("B", 4)
    A2 = A.copy()
    A2[3, 100] = np.nextafter(A2[3, 100], np.float32(10))      # same size, one bit apart
    ctx.sets["A2"] = A2
    u = [ctx.utts[0]]
    s0 = m.hotword_bank_stats()
    ctx.check(m.forward_ids(u, want_logp=True, hw_emb=A), 0, 0, "A")
    s1 = m.hotword_bank_stats()
    assert delta(s1, s0)["misses"] == 1 and delta(s1, s0)["hits"] == 0
    first = m.forward_ids(u, want_logp=True, hw_emb=A.copy())          # the same bytes from another buffer: found by content
    s2 = m.hotword_bank_stats()
    assert delta(s2, s1)["hits"] == 1 and delta(s2, s1)["misses"] == 0 and s2["bytes_in_use"] == SLAB
    ctx.check(first, 0, 0, "A")
    ctx.check(m.forward_ids(u, want_logp=True, hw_emb=A2), 0, 0, "A2")
    s3 = m.hotword_bank_stats()
    assert delta(s3, s2)["misses"] == 1 and delta(s3, s2)["hits"] == 0 and delta(s3, s2)["evictions"] == 0
    assert s3["bytes_in_use"] == 2 * SLAB
    ctx.check(m.forward_ids(u, want_logp=True, hw_emb=B), 0, 0, "B")    # a third set: A, the least recently used, goes
    s4 = m.hotword_bank_stats()
    assert delta(s4, s3)["misses"] == 1 and delta(s4, s3)["evictions"] == 1
    m.forward_ids(u, hw_emb=A2)
    s5 = m.hotword_bank_stats()
    assert delta(s5, s4)["hits"] == 1 and delta(s5, s4)["misses"] == 0          # A2 stayed
    ctx.check(m.forward_ids(u, want_logp=True, hw_emb=A), 0, 0, "A")    # the evicted set: a miss again, same answer
    s6 = m.hotword_bank_stats()
    assert delta(s6, s5)["misses"] == 1 and delta(s6, s5)["hits"] == 0 and delta(s6, s5)["evictions"] == 1
    big = ctx.hotwords("S301", 301)                          # three slabs: larger than the whole bound, served per call
    ctx.check(m.forward_ids([ctx.utts[4]], want_logp=True, hw_emb=big), 0, 4, "S301")
    s7 = m.hotword_bank_stats()
    d = delta(s7, s6)
    assert d["refused"] == 1 and d["per_call_forwards"] == 1 and d["evictions"] == 0 and s7["bytes_in_use"] <= 2 * SLAB
    # ... also beside a set the bank holds
    got = m.forward_ids([ctx.utts[4], ctx.utts[0]], want_logp=True, hw_sets=[big, A], set_of_utt=[0, 1])
    ctx.check(got, 0, 4, "S301")
    ctx.check(got, 1, 0, "A")
    m.set_hotword_bank_bytes(64 << 20)


def test_contextual_callers_merge_with_their_own_sets(ctx):
    """Eight threads, each with its own set and utterance, and a ninth without hotwords, on one handle with merging on.  The
    gather window (200 ms) is far longer than a forward: the first caller runs at once, whoever arrives while it runs is packed."""
    m = ctx.model
    m.set_hotword_bank_bytes(64 << 20)
    names = [f"M{i}" for i in range(8)]
    sets = [ctx.hotwords(n, 3 + 2 * i) for i, n in enumerate(names)]
    for i in range(8):
        ctx.ref(i, names[i])                                 # the oracle's answers first: the threads then start together
    m.set_batching(200000, 64)
    m.set_hotword_merging(True)
    slots0, bank0 = m.inflight_stats(), m.hotword_bank_stats()
    got = [None] * 9

    def work(i):
        got[i] = m.forward_ids([ctx.utts[i]], want_logp=True, hw_emb=sets[i] if i < 8 else None)
    err = run_threads(work, 9)
    slots1, bank1 = m.inflight_stats(), m.hotword_bank_stats()
    m.set_hotword_merging(False)
    m.set_batching(0, 32)
    assert all(e is None for e in err[:8]), err
    assert isinstance(err[8], ctx.pkg.PfhipError) and "hw_emb is null" in str(err[8])          # paraformer.cpp:516-520, that caller only
    for i in range(8):
        ctx.check(got[i], 0, i, names[i])
    fw = sum(a["forwards"] - b["forwards"] for a, b in zip(slots1, slots0))
    calls = sum(a["calls"] - b["calls"] for a, b in zip(slots1, slots0))
    assert calls == 9 and fw < calls, (fw, calls)
    d = delta(bank1, bank0)
    assert bank1["max_sets_in_forward"] > 1 and d["sets_in_forwards"] == 8 and d["forwards"] < 8, d


def test_inflight_contexts_keep_their_sets_pinned(pkg, ctx):
    """pfhip_set_inflight(3), six threads with distinct sets, three rounds each, a bank of three slabs: sets are evicted while
    other forwards are in flight; a slab a forward reads must never be handed out.  Run once."""
    m = pkg.ParaformerHip().InitAsr((ctx.man, ctx.blob))
    m.set_inflight(3)
    m.set_hotword_bank_bytes(3 * SLAB)
    names = [f"M{i}" for i in range(6)]
    sets = [ctx.hotwords(n, 3 + 2 * i) for i, n in enumerate(names)]
    for i in range(6):
        ctx.ref(i, names[i])
    got = [[None] * 3 for _ in range(6)]

    def work(i):
        for r in range(3):
            got[i][r] = m.forward_ids([ctx.utts[i]], want_logp=True, hw_emb=sets[i])
    err = run_threads(work, 6)
    st = m.hotword_bank_stats()
    used = sum(s["forwards"] > 0 for s in m.inflight_stats())
    m.close()
    assert all(e is None for e in err), err
    for i in range(6):
        for r in range(3):
            ctx.check(got[i][r], 0, i, names[i])
    assert st["forwards"] == 18 and st["evictions"] > 0 and st["bytes_in_use"] <= 3 * SLAB and used >= 2, (st, used)


def test_range_guard_rerun_sees_the_same_sets(pkg, weights_mod, ctx):
    """tests/test_gpu_range_guard.py's offset model (layer 0's projections into the residual stream x 2^18) with the bias decoder:
    6 x 22 s put the LayerNorm-folded GEMMs on the residual stream, the forward is redone on the exact kernels — with every
    utterance still attending to its own set."""
    cfg = weights_mod.small_config(enc_layers=3, dec_layers=1, vocab=257, contextual=1)
    man, blob = weights_mod.synth_weights(cfg, seed=61)
    blob = blob.copy()
    for name in ("enc.0.ffn2.w", "enc.0.ffn2.b", "enc.0.out.w", "enc.0.out.b"):
        meta = man["tensors"][name]
        n = int(np.prod(meta["shape"]))
        blob[meta["offset"] // 4: meta["offset"] // 4 + n] *= np.float32(2.0 ** 18)
    m = pkg.ParaformerHip().InitAsr((man, blob))
    W = P.Weights(man, blob)
    rng = np.random.default_rng(3)
    utts = [synth_pcm(i, 16000 * 22 + 97 * i, rng) for i in range(6)]
    sets = [m.CompileHotwordEmbedding([list(rng.integers(2, 257, 3)) for _ in range(k)]) for k in (5, 9)]
    of = [0, 1, 0, 1, 1, 0]
    got = m.forward_ids(utts, want_logp=True, hw_sets=sets, set_of_utt=of)
    assert m.debug_poke("range_fallbacks") >= 1
    for b in (0, 4):
        ref = P.forward_pcm(utts[b], W, hw_emb=sets[of[b]])
        assert int(got["n_fires"][b]) == ref["emb"].shape[0]
        assert np.abs(got["logp"][b] - ref["logp"]).max() < 1e-3
        assert_ids_match(got["ids"][b], ref, tie_gap=1e-3)
    other = P.forward_pcm(utts[0], W, hw_emb=sets[1])
    assert np.abs(got["logp"][0] - other["logp"]).max() > 1e-3
    m.close()


def test_decoder_threads_with_their_own_hotword_lists(pkg, weights_mod, tmp_path):
    """The handle API behind the server's decoder threads (`serve_threads` harness) on a reference-layout directory with
    model_eb.onnx: request r is served with hotword list r % 6, first alone, then from eight threads.  Every call's ids equal
    those of the same call made alone, and the concurrent calls were packed: more than one call per forward."""
    need_gpu()
    import importlib
    import ref_layout as RL
    conv = importlib.import_module(pkg.__name__ + ".convert")
    cfg = weights_mod.small_config(enc_layers=3, dec_layers=2, vocab=300, contextual=1)
    man, blob = weights_mod.synth_weights(cfg, seed=47)
    vocab = [chr(0x4E00 + i) for i in range(297)] + ["<s>", "</s>", "<unk>"]
    RL.write_asr_dir(str(tmp_path / "asr"), conv, man, blob, cfg, vocab_tokens=vocab)
    rng = np.random.default_rng(9)
    with open(tmp_path / "hotwords.txt", "w", encoding="utf-8") as f:
        for k in range(6):
            words = ["".join(vocab[int(j)] for j in rng.integers(0, 297, int(rng.integers(1, 5)))) for _ in range(3 + k)]
            f.write(" ".join(words) + "\n")
    exe = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "serve_threads")
    env = {k: v for k, v in os.environ.items() if not k.startswith("PFHIP_")}
    out = subprocess.run([exe, str(tmp_path / "asr"), "-", "8", "32", "2", "5", "1", str(tmp_path / "hotwords.txt")],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(r)
    assert r["hotword_lists"] == 6 and r["failures"] == 0
    assert r["mismatches"] == 0 and r["near_tie_flips"] == 0, r
    c = r["concurrent"]
    assert c["calls"] == 32 and c["forwards"] < c["calls"], c
    # six lists and the one-row set of the warm-up forward inside InitAsr: each is uploaded and projected once
    assert r["bank"]["max_sets_in_forward"] > 1 and 6 <= r["bank"]["misses"] <= 7 and r["bank"]["evictions"] == 0, r["bank"]
