"""GPU: pfhip_punc_* on CT-Transformers outside the 256 / 8 shape — the large model (d_model 516, twelve heads of 43, ffn 2048,
twelve blocks; the shape is recalled from the upstream config, no real file has been read) and three two-layer models of head
widths 24, 40 and 64 — against oracle.ct_transformer.

Logits: within 1e-3 of the oracle, the project's bar for these logits (tests/test_gpu_punc.py).
Punctuation ids, the tie rule: a row whose oracle top-2 gap over the first n_punc - 1 classes is below 2e-3 may take the runner-up
(two logits that are each off by up to the tolerance can swap only when they are closer than that); every other row must match
exactly, and the rule may excuse at most 1 % of the rows of a test function's cases taken together.  On the CPU the oracle has
2 such rows of the 403 offline rows, 1 and 0 of the 305 online rows (sanm_shift 0 and 5) and 1, 0, 0 of the 229 rows of the
other widths.

Each case prints its largest logit error."""
import numpy as np
import pytest

from oracle import ct_transformer as C
from oracle import paraformer as P

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VOCAB = 3000
LOGIT_TOL = 1e-3
TIE_GAP = 2e-3
LARGE = dict(vocab=VOCAB, d_model=516, n_head=12, ffn=2048, layers=12)
OFFLINE_N = [1, 20, 33, 64, 65, 220]
ONLINE_CASES = [(30, 12), (30, 0), (30, 30), (75, 2), (140, 100)]
WIDTH_N = [1, 33, 65, 130]
WIDTHS = [(dict(d_model=96, n_head=4, ffn=128, layers=2), 11), (dict(d_model=120, n_head=3, ffn=256, layers=2), 12),
          (dict(d_model=192, n_head=3, ffn=256, layers=2), 13)]


class Tally:
    """The tie rule's books for one test function: rows seen, rows excused, and the cap the rows of all its cases set."""

    def __init__(self, total_rows):
        self.cap = total_rows // 100
        self.excused = 0

    def check_ids(self, got, ref_logits, n_punc, what):
        lg = np.asarray(ref_logits)[:, :n_punc - 1]
        want = np.argmax(lg, axis=-1)
        for r, (a, b) in enumerate(zip(got, want)):
            if int(a) == int(b):
                continue
            order = np.argsort(-lg[r], kind="stable")
            gap = float(lg[r][order[0]] - lg[r][order[1]])
            assert gap < TIE_GAP and int(a) == int(order[1]), f"{what} row {r}: got {a}, oracle {b} (top-2 gap {gap:.2e})"
            self.excused += 1
        assert self.excused <= self.cap, f"{what}: the tie rule has excused {self.excused} rows, the cap is {self.cap}"


def make(pkg, weights_mod, cfg_over, seed):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    cfg = dict(weights_mod.CT_TRANSFORMER, **cfg_over)
    man, blob = weights_mod.synth_punc_weights(cfg, seed=seed)
    return pkg.CTTransformerHip().InitPunc((man, blob)), P.Weights(man, blob)


@pytest.fixture(scope="module")
def large(pkg, weights_mod):
    h, W = make(pkg, weights_mod, LARGE, 2468)
    yield h, W
    h.close()


@pytest.fixture(scope="module")
def offline_tally():
    return Tally(sum(OFFLINE_N))


@pytest.mark.parametrize("n", OFFLINE_N)
def test_large_offline_matches_oracle(large, offline_tally, n):
    h, W = large
    ids = np.random.default_rng(n).integers(0, VOCAB, n).astype(np.int32)
    got_p, got_l = h.Infer(ids, want_logits=True)
    ref_l, _ = C.infer(ids, W)
    err = float(np.abs(got_l - ref_l).max())
    print(f"516 / 12 / 2048 x 12 offline, n = {n}: max logit err {err:.3e}")
    assert err < LOGIT_TOL, (n, err)
    offline_tally.check_ids(got_p, ref_l, W.cfg["n_punc"], f"offline n = {n}")
    assert got_p.max() <= 4            # class 5 can never be chosen: Argmax over CANDIDATE_NUM-1 classes


@pytest.mark.parametrize("shift,seed", [(0, 7), (5, 12)])
def test_large_online_with_vad_mask(pkg, weights_mod, shift, seed):
    h, W = make(pkg, weights_mod, dict(LARGE, sanm_shift=shift), seed)
    tally = Tally(sum(n for n, _ in ONLINE_CASES))
    for n, pos in ONLINE_CASES:
        ids = np.random.default_rng(40 + n).integers(0, VOCAB, n).astype(np.int32)
        gp, gl = h.Infer(ids, want_logits=True, nCacheSize=pos)
        rl, _ = C.forward_online(ids, W, pos)
        err = float(np.abs(gl - rl).max())
        print(f"516 / 12 / 2048 x 12 online, sanm_shift {shift}, n = {n}, cache {pos}: max logit err {err:.3e}")
        assert err < LOGIT_TOL, (n, pos, err)
        tally.check_ids(gp, rl, W.cfg["n_punc"], f"online shift {shift} n = {n} cache {pos}")
    # the mask matters: with a cut in the middle the early tokens' scores differ from the unmasked run
    ids = np.random.default_rng(40).integers(0, VOCAB, 60).astype(np.int32)
    _, a = h.Infer(ids, want_logits=True, nCacheSize=30)
    _, b = h.Infer(ids, want_logits=True, nCacheSize=0)
    assert np.abs(a[:20] - b[:20]).max() > 1e-3
    h.close()


@pytest.fixture(scope="module")
def widths_tally():
    return Tally(len(WIDTHS) * sum(WIDTH_N))


@pytest.mark.parametrize("cfg_over,seed", WIDTHS, ids=["dk24", "dk40", "dk64"])
def test_other_head_widths(pkg, weights_mod, widths_tally, cfg_over, seed):
    h, W = make(pkg, weights_mod, dict(cfg_over, vocab=VOCAB), seed)
    for n in WIDTH_N:
        ids = np.random.default_rng(n).integers(0, VOCAB, n).astype(np.int32)
        got_p, got_l = h.Infer(ids, want_logits=True)
        ref_l, _ = C.infer(ids, W)
        err = float(np.abs(got_l - ref_l).max())
        print(f"{cfg_over['d_model']} / {cfg_over['n_head']} / {cfg_over['ffn']} x 2, n = {n}: max logit err {err:.3e}")
        assert err < LOGIT_TOL, (cfg_over, n, err)
        widths_tally.check_ids(got_p, ref_l, W.cfg["n_punc"], f"d_model {cfg_over['d_model']} n = {n}")
    h.close()


def test_large_batched_infer_equals_separate_calls(large):
    h, _ = large
    rng = np.random.default_rng(99)
    seqs = [rng.integers(0, VOCAB, n).astype(np.int32) for n in (1, 20, 33, 64, 7)]
    got = h.InferBatch(seqs)
    for x, g in zip(seqs, got):
        assert np.array_equal(g, h.Infer(x))


def test_workspace_growth_keeps_the_pad_columns_zero(pkg, weights_mod):
    """A fresh handle, a short call and then one of 450 ids: the activations outgrow their first allocation (512 rows of 640
    floats is more than the 1 MiB a buffer starts with), so the context and the memory block land in fresh memory whose pad columns
    [516, 640) the GEMMs read.  At this size the QKV and FFN1 GEMMs also run the split-operand kernels.  Same bars, same tie rule."""
    h, W = make(pkg, weights_mod, LARGE, 2468)
    h.Infer(np.arange(5, dtype=np.int32))
    n = 450
    ids = np.random.default_rng(n).integers(0, VOCAB, n).astype(np.int32)
    got_p, got_l = h.Infer(ids, want_logits=True)
    ref_l, _ = C.infer(ids, W)
    err = float(np.abs(got_l - ref_l).max())
    print(f"516 / 12 / 2048 x 12 offline after a reallocation, n = {n}: max logit err {err:.3e}")
    assert np.isfinite(got_l).all() and err < LOGIT_TOL, err
    Tally(n).check_ids(got_p, ref_l, W.cfg["n_punc"], f"offline n = {n}")
    h.close()


def test_large_add_punc_mini_sentences(large):
    """pfhip_punc_add_punc on 130 ids against the oracle's restatement of AddPunc, under the tie rule: the outputs are walked in
    order, each with the oracle row it came from; at the first difference that row must be one the rule excuses, and nothing
    after it is compared (what the later mini-sentences carry depends on it)."""
    h, W = large
    n_punc = W.cfg["n_punc"]
    ids = np.random.default_rng(130).integers(0, VOCAB, 130).astype(np.int32)
    rows = []                                   # per Infer call of the oracle: the logits of its rows

    def infer(inp):
        lg, p = C.infer(np.asarray(inp, np.int32), W)
        rows.append(lg[:, :n_punc - 1])
        return list(p)

    ref = C.add_punc_ids(ids, W, infer_fn=infer)
    got = [int(v) for v in h.AddPuncIds(ids)]
    # where each output position comes from: call k keeps its first rows, all but what call k + 1 carries over (its length minus
    # the fresh tokens it takes); the last call keeps all of its rows
    origin = []
    for k, lg in enumerate(rows):
        carried = 0 if k == len(rows) - 1 else rows[k + 1].shape[0] - min(20, len(ids) - 20 * (k + 1))
        origin += [(k, r) for r in range(lg.shape[0] - carried)]
    for i, (a, b) in enumerate(zip(got, ref)):
        if a == b:
            continue
        assert i < len(origin), f"position {i}: got {a}, oracle {b} (the appended period)"
        k, r = origin[i]
        order = np.argsort(-rows[k][r], kind="stable")
        gap = float(rows[k][r][order[0]] - rows[k][r][order[1]])
        assert gap < TIE_GAP and a == int(order[1]), f"position {i} (call {k} row {r}): got {a}, oracle {b} (top-2 gap {gap:.2e})"
        break                                   # one excused row: the comparison ends here
    else:
        assert len(got) == len(ref)
    assert len(ref) in (130, 131) and ref[-1] in (3, 4)


@pytest.mark.parametrize("over", [dict(d_model=520, n_head=8), dict(d_model=1028, n_head=257), dict(d_model=258, n_head=6)],
                         ids=["dk65", "d1028", "d258"])
def test_widths_outside_the_range_are_refused_at_create(pkg, weights_mod, over):
    cfg = dict(weights_mod.CT_TRANSFORMER, vocab=50, ffn=128, layers=1, **over)
    man, blob = weights_mod.synth_punc_weights(cfg, seed=3)
    with pytest.raises(pkg.PfhipError, match=r"d_model % 4 == 0, d_model <= 1024.*1 <= d_model / n_head <= 64"):
        pkg.CTTransformerHip().InitPunc((man, blob))
