"""GPU: the offline forward through the C ABI (include/pfhip.h) against the oracle and the reference's
golden vectors.  BASELINE.json tolerance: tokens identical, log-probs within 1e-3 (fp32)."""
import os

import numpy as np
import pytest

from conftest import assert_ids_match, synth_pcm
from oracle import frontend as fe
from oracle import paraformer as P

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOGP_TOL = 1e-3          # BASELINE.json north_star: "logits within 1e-3 fp32"
FEAT_TOL = 2e-5          # log-mel after CMVN(istd 0.3): GPU logf / fp64 FFT rounding, well under SURVEY's 1e-4


@pytest.fixture(scope="module")
def small(pkg, weights_mod):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    cfg = weights_mod.small_config()
    man, blob = weights_mod.synth_weights(cfg)
    model = pkg.ParaformerHip().InitAsr((man, blob))
    yield model, P.Weights(man, blob)
    model.close()


@pytest.mark.parametrize("name", ["fbank_synth", "fbank_xmov", "fbank_floor", "fbank_stevejobs_10s", "fbank_number", "fbank_fullscale"])
def test_feats_match_reference_golden(small, name):
    """fbank from the REFERENCE's knf (golden) -> oracle LFR/CMVN  vs  the fused HIP kernel."""
    model, W = small
    g = np.load(os.path.join(GOLD, name + ".npz"))
    got = model.extract_feats([g["pcm"].astype(np.float32) / 32768])[0]
    ref = fe.lfr_cmvn(g["fbank"], W["cmvn.mean"], W["cmvn.istd"])
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() < FEAT_TOL


def test_feats_ragged_batch_and_edges(small):
    model, W = small
    rng = np.random.default_rng(1)
    lens = [399, 400, 559, 560, 1359, 1360, 16000, 80000, 0, 48123]
    utts = [synth_pcm(i, n, rng) for i, n in enumerate(lens)]
    got = model.extract_feats(utts)
    for u, g_ in zip(utts, got):
        ref = fe.extract_feats(u, W["cmvn.mean"], W["cmvn.istd"])
        assert g_.shape == ref.shape
        if ref.size:
            assert np.abs(g_ - ref).max() < FEAT_TOL


def test_feats_more_than_64_utterances(small):
    """The kernel finds a frame's utterance by ballots over the frame-offset table, 64 entries at a time: 150 utterances (three
    table chunks), odd sample counts (unaligned utterance starts), empty and too-short ones in between."""
    model, W = small
    rng = np.random.default_rng(7)
    lens = [int(v) for v in rng.integers(300, 4001, size=150)]
    for i in (0, 63, 64, 65, 127, 128, 149):
        lens[i] = [0, 399, 401, 1361, 0, 977, 2001][(i * 7) % 7]
    utts = [synth_pcm(i, n, rng) for i, n in enumerate(lens)]
    got = model.extract_feats(utts)
    assert len(got) == len(utts)
    for u, g_ in zip(utts, got):
        ref = fe.extract_feats(u, W["cmvn.mean"], W["cmvn.istd"])
        assert g_.shape == ref.shape
        if ref.size:
            assert np.abs(g_ - ref).max() < FEAT_TOL


def test_forward_ragged_batch_matches_oracle(small):
    """Mixed lengths incl. an utterance too short for one window; per-stage + token-for-token."""
    model, W = small
    rng = np.random.default_rng(20251114)
    lens = [32000, 80123, 399, 48000, 5 * 16000, 16000 * 7 + 5, 9000]
    utts = [synth_pcm(i, n, rng) for i, n in enumerate(lens)]
    got = model.forward_ids(utts, want_logp=True)
    M = int(got["n_frames"].sum())
    enc = model.get_tensor("enc", M * 512).reshape(M, 512)
    alphas = model.get_tensor("alphas", M)
    ro = 0
    for b, u in enumerate(utts):
        ref = P.forward_pcm(u, W)
        T = ref["feats"].shape[0]
        assert got["n_frames"][b] == T
        if T == 0:
            assert got["token_num"][b] == 0 and got["n_fires"][b] == 0 and len(got["ids"][b]) == 0
            continue
        assert np.abs(enc[ro:ro + T] - ref["enc"]).max() < 1e-4
        assert np.abs(alphas[ro:ro + T] - ref["alphas"][:T]).max() < 1e-5
        assert got["n_fires"][b] == ref["emb"].shape[0]
        assert got["token_num"][b] == ref["token_num"]
        assert np.abs(got["logp"][b] - ref["logp"]).max() < LOGP_TOL
        assert list(got["ids"][b]) == list(ref["ids"])
        ro += T


def test_batch_composition_invariance(small):
    """An utterance's result must not depend on what it is batched with (packed layout, masks)."""
    model, _ = small
    rng = np.random.default_rng(5)
    utts = [synth_pcm(i, n, rng) for i, n in enumerate([40000, 23456, 64000])]
    alone = [model.forward_ids([u], want_logp=True) for u in utts]
    together = model.forward_ids(utts, want_logp=True)
    for b in range(3):
        assert list(alone[b]["ids"][0]) == list(together["ids"][b])
        assert np.abs(alone[b]["logp"][0] - together["logp"][b]).max() < 1e-4


def test_model_forward_contract(small):
    """Model::Forward returns batch_in strings; too-short audio gives "" (paraformer.cpp:477-480)."""
    model, _ = small
    rng = np.random.default_rng(6)
    res = model.Forward([synth_pcm(0, 32000, rng), np.zeros(100, np.float32)], batch_in=2)
    assert len(res) == 2 and res[1] == "" and len(res[0]) > 0


def test_errors_are_loud(pkg, weights_mod):
    cfg = weights_mod.small_config(enc_layers=1, dec_layers=0)
    man, blob = weights_mod.synth_weights(cfg)
    bad = dict(man, tensors={k: v for k, v in man["tensors"].items() if k != "enc.0.out.w"})
    with pytest.raises(pkg.PfhipError, match="missing tensor"):
        pkg.ParaformerHip().InitAsr((bad, blob))
    cfg2 = dict(cfg, n_head=8)
    with pytest.raises(pkg.PfhipError):
        pkg.ParaformerHip().InitAsr((dict(man, config=cfg2), blob))
    m = pkg.ParaformerHip().InitAsr((man, blob))
    with pytest.raises(pkg.PfhipError):
        m.forward_ids([np.zeros(32000, np.float32)], max_tokens=0)   # capacity error, not silent truncation
    m.close()


def test_refused_load_gives_its_memory_back(pkg, weights_mod):
    """A manifest that build_model refuses AFTER the blob went up (a tensor missing, a tensor of another shape) must leave no HBM
    behind: everything the loader had allocated goes back through the destructors of what it was building.  Free memory after each
    refused load is at least what it was before, minus the 8 MiB that test_gpu_contexts.py allows for "costs next to nothing"; the
    blob is 80 MB, so a loader that drops it on the floor misses by ten times the allowance."""
    cfg = weights_mod.small_config(enc_layers=5, dec_layers=1)
    man, blob = weights_mod.synth_weights(cfg)
    assert blob.nbytes >= 64 << 20
    pkg.ParaformerHip().InitAsr((man, blob)).close()          # the runtime's one-time allocations fall outside the window
    tensors, name = man["tensors"], "enc.4.ffn2.w"
    missing = dict(man, tensors={k: v for k, v in tensors.items() if k != name})
    reshaped = dict(man, tensors=dict(tensors, **{name: dict(tensors[name], shape=tensors[name]["shape"][::-1])}))
    for bad, why in ((missing, "missing tensor"), (reshaped, "unexpected shape")):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        with pytest.raises(pkg.PfhipError, match=why):
            pkg.ParaformerHip().InitAsr((bad, blob))
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        print(f"refused load ({why}): blob {blob.nbytes >> 20} MiB, free before {free0 >> 20} MiB, after {free1 >> 20} MiB")
        assert free1 >= free0 - (8 << 20), (why, free0 - free1, blob.nbytes)


def test_full_size_properties(pkg, weights_mod):
    """BASELINE configs[1] shapes (full Paraformer-large, 30-s utterances) through size-independent
    properties: deterministic, batch-order equivariant, log-probs normalised, token_num == fires."""
    cfg = dict(weights_mod.PARAFORMER_LARGE)
    man, blob = weights_mod.synth_weights(cfg)
    model = pkg.ParaformerHip().InitAsr((man, blob))
    rng = np.random.default_rng(20251114)
    utts = [synth_pcm(i, 480000, rng) for i in range(4)]
    a = model.forward_ids(utts, want_logp=True)
    b = model.forward_ids(utts[::-1])
    assert list(a["n_frames"]) == [500] * 4
    for i in range(4):
        assert list(a["ids"][i]) == list(b["ids"][3 - i])
        assert a["token_num"][i] == a["n_fires"][i] and a["token_num"][i] > 0
        assert np.abs(np.exp(a["logp"][i].astype(np.float64)).sum(-1) - 1).max() < 1e-4
        assert np.array_equal(a["logp"][i].argmax(-1)[:len(a["ids"][i])], a["ids"][i])
    c = model.forward_ids(utts)
    assert all(list(x) == list(y) for x, y in zip(a["ids"], c["ids"]))
    model.close()


def test_cross_request_batching_matches_separate_calls(small):
    """pfhip_set_batching: concurrent callers (the server's decoder threads) are merged into one packed forward;
    every caller must get exactly what a call on its own returns."""
    import threading
    model, _ = small
    rng = np.random.default_rng(31)
    reqs = [[synth_pcm(i * 3 + j, int(rng.integers(8000, 70000)), rng) for j in range(1 + i % 3)] for i in range(7)]
    alone = [model.forward_ids(r, want_logp=(i % 2 == 0)) for i, r in enumerate(reqs)]
    model.set_batching(20000, 16)
    got = [None] * len(reqs)
    errs = []

    def work(i):
        try:
            got[i] = model.forward_ids(reqs[i], want_logp=(i % 2 == 0))
        except Exception as e:          # noqa: BLE001
            errs.append(e)

    ths = [threading.Thread(target=work, args=(i,)) for i in range(len(reqs))]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    model.set_batching(0, 32)
    assert not errs, errs
    for a, g in zip(alone, got):
        assert list(a["token_num"]) == list(g["token_num"]) and list(a["n_frames"]) == list(g["n_frames"])
        for x, y in zip(a["ids"], g["ids"]):
            assert list(x) == list(y)
        if a["logp"] is not None:
            for x, y in zip(a["logp"], g["logp"]):
                assert np.abs(x - y).max() < 1e-4


def test_full_size_batch_matches_oracle(pkg, weights_mod):
    """BASELINE configs[1] exactly — Paraformer-large, 32 x 30 s in one packed forward (M = 16000: the encoder on plane-image
    operands) — against the CPU restatement for ALL 32 utterances (oracle on a thread pool, one BLAS thread each): token ids
    identical up to near-ties, log-probs within the 1e-3 that north_star states; the assertion message carries the maximum and the
    95th percentile of the per-utterance log-prob error."""
    from concurrent.futures import ThreadPoolExecutor
    cfg = dict(weights_mod.PARAFORMER_LARGE)
    man, blob = weights_mod.synth_weights(cfg)
    model = pkg.ParaformerHip().InitAsr((man, blob))
    W = P.Weights(man, blob)
    rng = np.random.default_rng(20251114)
    utts = [synth_pcm(i, 480000, rng) for i in range(32)]
    got = model.forward_ids(utts, want_logp=True)
    # the encoder ran on plane-image operands (gemm_p3.hip) — unless this process was started with one of the knobs that keep the
    # GEMMs or the attention on another form (test_gpu_ops.py runs this test that way too)
    other_form = any(os.environ.get(k) == "0" for k in ("PFHIP_GEMM_X3", "PFHIP_GEMM_X6", "PFHIP_ATT_X3", "PFHIP_ATT_X6", "PFHIP_PLANES"))
    assert model._lib.pfhip_debug_poke(model.handle, b"plane_forwards", 0) == (0 if other_form else 1)
    assert model.debug_poke("range_fallbacks") == 0 and model.debug_poke("always_exact") == 0
    # ~7000 token rows: the decoder's K/V projections, FFNs and output projections ran on plane images too (round 4)
    assert model.debug_poke("dec_plane_forwards") == (0 if other_form else 1)
    try:
        from threadpoolctl import threadpool_limits
        limiter = threadpool_limits(limits=1)
    except Exception:                      # noqa: BLE001 - the pool still works with threaded BLAS, only slower
        limiter = None
    workers = max(1, min(12, (os.cpu_count() or 4) - 2))
    with ThreadPoolExecutor(workers) as pool:
        refs = list(pool.map(lambda u: P.forward_pcm(u, W), utts))
    if limiter is not None:
        limiter.restore_original_limits()
    errs = []
    for i, ref in enumerate(refs):
        assert int(got["token_num"][i]) == ref["token_num"], i
        assert int(got["n_fires"][i]) == ref["emb"].shape[0], i
        assert_ids_match(got["ids"][i], ref)
        assert ref["logp"].shape[0] > 50
        errs.append(float(np.abs(got["logp"][i] - ref["logp"]).max()))
    errs = np.asarray(errs)
    msg = f"log-prob error over 32 utterances: max {errs.max():.3e}, 95th percentile {np.percentile(errs, 95):.3e}, median {np.median(errs):.3e}"
    print(msg)
    # north_star's bound, and what fp32-grade arithmetic end to end actually gives: two equally exact GPU paths (plane-image
    # operands, fp32 operands: tools/planes_check.py) sit 1e-5 .. 1e-4 from the restatement — rounding noise through 50 layers
    assert errs.max() < 1e-3, msg
    assert np.percentile(errs, 95) < 2e-4, msg
    model.close()


@pytest.mark.parametrize("n_utts,check", [(36, (0, 13, 35)), (5, (0, 4)), (12, (0, 11))])
def test_layernorm_folded_into_the_gemms_with_strong_gamma_beta(pkg, weights_mod, n_utts, check):
    """Batches of >= 1536 rows take the fused encoder path (forward.cpp `fuse_ln`): the GEMMs that write the residual stream leave
    per-tile row statistics, the GEMMs that read it normalise on load with gamma folded into their weights and beta into their
    bias.  Here gamma in [0.5, 1.5] and beta in [-0.5, 0.5] for every LayerNorm (the default synthetic weights keep them within
    5 % of 1 / 0), 36 x 30 s = 18000 encoder rows and > 4096 decoder rows (so the decoder's norm1 -> FFN1 and ffn_norm -> FFN2
    folds run too) and 5 x 30 s = 2500 rows (the 64-row tiles of the same kernels), against the oracle's explicit two-pass
    LayerNorm."""
    cfg = weights_mod.small_config(enc_layers=4, dec_layers=2, vocab=700)
    man, blob = weights_mod.synth_weights(cfg, seed=77)
    rng = np.random.default_rng(5)
    for name, t in man["tensors"].items():
        if "norm" in name and (name.endswith(".g") or name.endswith(".b")):
            o, n = t["offset"] // 4, int(np.prod(t["shape"]))
            blob[o:o + n] = (rng.uniform(0.5, 1.5, n) if name.endswith(".g") else rng.uniform(-0.5, 0.5, n)).astype(np.float32)
    model = pkg.ParaformerHip().InitAsr((man, blob))
    W = P.Weights(man, blob)
    utts = [synth_pcm(i, 480000 - 1234 * (i % 9), rng) for i in range(n_utts)]
    got = model.forward_ids(utts, want_logp=True)
    planes = model._lib.pfhip_debug_poke(model.handle, b"plane_forwards", 0)
    # 18000 rows: LayerNorm folded into the plane-operand GEMMs on 128-row tiles; 6000 rows: the same on 64-row tiles for the
    # N = 512 launches; 2500 rows: fp32 operands
    other_form = any(os.environ.get(k) == "0" for k in ("PFHIP_GEMM_X3", "PFHIP_GEMM_X6", "PFHIP_ATT_X3", "PFHIP_ATT_X6", "PFHIP_PLANES"))
    assert planes == (0 if n_utts == 5 or other_form else 1)
    if n_utts == 36:
        assert int(sum(got["n_frames"])) >= 4096 and int(sum(got["n_fires"])) >= 4096
    elif n_utts == 12:      # decoder rows between the two thresholds: its folded FFN2 (LayerNorm over 2048 columns) on 64-row tiles
        assert int(sum(got["n_frames"])) >= 4096 and 1536 <= int(sum(got["n_fires"])) < 4096
    else:
        assert 1536 <= int(sum(got["n_frames"])) < 4096
    enc = model.get_tensor("enc", int(sum(got["n_frames"])) * 512).reshape(-1, 512)
    o = 0
    for i, u in enumerate(utts):
        T = int(got["n_frames"][i])
        if i in check:
            ref = P.forward_pcm(u, W)
            assert np.abs(enc[o:o + T] - ref["enc"]).max() < 2e-4, i
            assert int(got["token_num"][i]) == ref["token_num"]
            assert_ids_match(got["ids"][i], ref)          # utterance 4 of the 5-utterance case has a 1.2e-5 tie at row 101
            assert np.abs(got["logp"][i] - ref["logp"]).max() < 1e-3
        o += T
    model.close()
