"""GPU: the small Paraformer — d_model 320, four attention heads of 80, FFN 1280 in encoder and decoder, the widths of the online
model the reference's 2-pass launch scripts stream with (websocket/run_server_2pass.sh:27-28; the widths themselves are upstream
knowledge no file here confirms) — through the offline forward, the range guard's exact re-run, the chunk-streaming path and the
reference's file layout, against oracle/paraformer.py and oracle/paraformer_online.py.

Six utterances of T = 50, 118, 200, 150, 367 and 33 LFR frames (367 is more than one 256-query block of attention_h80.hip, 33 is below
the 64-query switch onto the fp32-MFMA kernel), 251 tokens.  The oracle's smallest top-2 log-prob gap over those 251 rows is 2.1e-4:
no row qualifies for assert_ids_match's 1e-4 tie rule, so the ids must be identical."""
import importlib

import numpy as np
import pytest

import ref_layout as RL
from conftest import assert_ids_match, synth_pcm
from oracle import paraformer as P
from oracle import paraformer_online as PO

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D = 320
LENS = [48077, 113234, 192005, 144311, 352097, 32000]
FRAMES = [50, 118, 200, 150, 367, 33]


@pytest.fixture(scope="module")
def small320(pkg, weights_mod):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    cfg = weights_mod.small_config_320()
    man, blob = weights_mod.synth_weights(cfg, seed=320)
    W = P.Weights(man, blob)
    rng = np.random.default_rng(80)
    utts = [synth_pcm(i, n, rng) for i, n in enumerate(LENS)]
    refs = [P.forward_pcm(u, W) for u in utts]                  # computed once, shared, never modified
    model = pkg.ParaformerHip().InitAsr((man, blob))
    yield dict(cfg=cfg, man=man, blob=blob, W=W, utts=utts, refs=refs, model=model)
    model.close()


def test_oracle_recipe(small320):
    """What the module docstring states about the inputs (CPU only: guards the margins the other tests lean on)."""
    refs = small320["refs"]
    assert [r["feats"].shape[0] for r in refs] == FRAMES
    assert sum(len(r["ids"]) for r in refs) == 251
    gap = min(float(np.sort(row)[-1] - np.sort(row)[-2]) for r in refs for row in np.asarray(r["logp"]))
    assert gap > 1e-4, gap


def check_against_oracle(got, s, logp_tol=1e-3):
    worst = 0.0
    for b, ref in enumerate(s["refs"]):
        assert int(got["n_frames"][b]) == FRAMES[b]
        assert int(got["n_fires"][b]) == ref["emb"].shape[0] and int(got["token_num"][b]) == ref["token_num"]
        worst = max(worst, float(np.abs(got["logp"][b] - ref["logp"]).max()))
        assert_ids_match(got["ids"][b], ref)
        assert list(got["ids"][b]) == [int(x) for x in ref["ids"]]
    print(f"small Paraformer: log-prob max abs err {worst:.3e}")
    assert worst < logp_tol, worst


def test_one_packed_forward_of_all_six(small320):
    s = small320
    model = s["model"]
    assert model._lib.pfhip_head_dim(model._h) == 80 and model._lib.pfhip_d_model(model._h) == D
    got = model.forward_ids(s["utts"], want_logp=True)
    M = int(got["n_frames"].sum())
    assert M == sum(FRAMES)
    enc = model.get_tensor("enc", M * D).reshape(M, D)
    alphas = model.get_tensor("alphas", M)
    ro = 0
    for ref, T in zip(s["refs"], FRAMES):
        e_enc = float(np.abs(enc[ro:ro + T] - ref["enc"]).max())
        e_al = float(np.abs(alphas[ro:ro + T] - ref["alphas"][:T]).max())
        print(f"small Paraformer: T = {T}: enc err {e_enc:.3e}, alphas err {e_al:.3e}")
        assert e_enc < 1e-4 and e_al < 1e-5
        ro += T
    check_against_oracle(got, s)
    assert model.debug_poke("range_fallbacks") == 0 and model.debug_poke("always_exact") == 0


def test_batch_composition(small320):
    s = small320
    together = s["model"].forward_ids(s["utts"], want_logp=True)
    for b, u in enumerate(s["utts"]):
        alone = s["model"].forward_ids([u], want_logp=True)
        assert list(alone["ids"][0]) == list(together["ids"][b])
        assert np.abs(alone["logp"][0] - together["logp"][b]).max() < 1e-4


def test_range_guard_reruns_on_the_exact_kernels(small320):
    s = small320
    model = s["model"]
    before = model.debug_poke("range_fallbacks")
    assert 1 < model.debug_poke("static_bound") < 32768             # the static bound at load holds for the new width
    assert model.debug_poke("range_flag", 1) == 0
    got = model.forward_ids(s["utts"], want_logp=True)
    assert model.debug_poke("range_fallbacks") == before + 1
    check_against_oracle(got, s)
    got = model.forward_ids(s["utts"], want_logp=True)
    assert model.debug_poke("range_fallbacks") == before + 1        # one forward only
    check_against_oracle(got, s)


def test_streaming_one_connection(pkg, small320):
    s = small320
    W, vocab = s["W"], s["cfg"]["vocab"]
    rng = np.random.default_rng(21)
    pcm = synth_pcm(9, 9600 * 5 + 3000, rng)
    on = PO.ParaformerOnline(W)
    hip = pkg.ParaformerOnlineHip(s["model"])
    hip.set_debug(True)
    pos, total = 0, 0
    for n, fin in [(9600, False)] * 5 + [(3000, True)]:
        seg = pcm[pos:pos + n]
        pos += n
        before = len(on.chunk_log)
        ref_ids = on.Forward(seg, fin)
        got_ids = hip.Forward(seg, input_finished=fin)
        assert got_ids == ref_ids, (n, fin, got_ids, ref_ids)
        total += len(got_ids)
        if len(on.chunk_log) > before and on.chunk_log[-1]["logp"] is not None:
            last = on.chunk_log[-1]
            logp = hip.get_tensor("logp", 128 * vocab).reshape(-1, vocab)
            assert logp.shape == last["logp"].shape
            err = float(np.abs(logp - last["logp"]).max())
            print(f"small Paraformer stream: chunk log-prob err {err:.3e}")
            assert err < 5e-4, err
    assert total > 0
    hip.close()


def test_streaming_twelve_connections_in_one_round(pkg, small320):
    model = small320["model"]
    rng = np.random.default_rng(22)
    waves = [synth_pcm(i, 9600 * (2 + i % 3) + 111 * i, rng) for i in range(12)]
    plan = lambda n: [(k, min(k + 9600, n)) for k in range(0, n, 9600)]
    alone = []
    for w in waves:
        st = pkg.ParaformerOnlineHip(model)
        ids, p = [], plan(len(w))
        for j, (a, b) in enumerate(p):
            ids += st.Forward(w[a:b], input_finished=(j == len(p) - 1))
        alone.append(ids)
        st.close()
    streams = [pkg.ParaformerOnlineHip(model) for _ in waves]
    plans = [plan(len(w)) for w in waves]
    got = [[] for _ in waves]
    for j in range(max(len(p) for p in plans)):
        act = [i for i, p in enumerate(plans) if j < len(p)]
        res = pkg.ParaformerOnlineHip.forward_batch([streams[i] for i in act], [waves[i][plans[i][j][0]:plans[i][j][1]] for i in act],
                                                    [j == len(plans[i]) - 1 for i in act])
        for i, r in zip(act, res):
            got[i] += r
    for st in streams:
        st.close()
    assert got == alone and sum(len(x) for x in alone) > 10


def test_reference_file_layout(pkg, small320, tmp_path):
    """The 320-wide model as an online directory of the reference (model.onnx + decoder.onnx + am.mvn + config.yaml), loaded in C++."""
    s = small320
    conv = importlib.import_module(pkg.__name__ + ".convert")
    d = tmp_path / "small-online"
    RL.write_asr_dir(str(d), conv, s["man"], s["blob"], s["cfg"], online=True)
    model = pkg.ParaformerHip().InitAsr(str(d / "model.onnx"), str(d / "am.mvn"), str(d / "config.yaml"), str(d / "tokens.json"),
                                        second_model=str(d / "decoder.onnx"))
    assert model._lib.pfhip_head_dim(model._h) == 80 and model._lib.pfhip_d_model(model._h) == D
    assert model.cfg["d_model"] == D and model.cfg["n_head"] == 4 and model.cfg["ffn"] == 1280 and model.cfg["dec_ffn"] == 1280
    picks = (0, 5)
    got = model.forward_ids([s["utts"][b] for b in picks], want_logp=True)
    for k, b in enumerate(picks):
        assert list(got["ids"][k]) == [int(x) for x in s["refs"][b]["ids"]]
        assert np.abs(got["logp"][k] - s["refs"][b]["logp"]).max() < 1e-3
    model.close()


@pytest.mark.parametrize("head", ["contextual", "timestamp"])
def test_hotword_and_timestamp_heads_are_refused_at_this_width(pkg, weights_mod, head):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    cfg = weights_mod.small_config_320(enc_layers=1, dec_layers=1, vocab=53, **{head: 1})
    man, blob = weights_mod.synth_weights(cfg, seed=7)
    with pytest.raises(pkg.PfhipError, match="head width.*80"):
        pkg.ParaformerHip().InitAsr((man, blob))


def test_head_width_64_is_still_refused(pkg, weights_mod):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    cfg = weights_mod.small_config(enc_layers=1, dec_layers=0)
    man, blob = weights_mod.synth_weights(cfg)
    with pytest.raises(pkg.PfhipError, match="d_model/n_head == 128 or 80"):
        pkg.ParaformerHip().InitAsr((dict(man, config=dict(cfg, n_head=8)), blob))
