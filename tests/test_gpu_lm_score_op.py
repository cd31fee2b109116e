"""GPU: sentences scored by the token n-gram language model (csrc/lm_score.hip, and with it csrc/lm_step.h on its own) through
pfhip_op_lm_score, against the plain-Python restatement tests/lm_ref.py: per-token weights, the end-of-sentence weight and the totals
are EQUAL BIT FOR BIT — the device only adds baked float32 weights, in a stated order.

B = 5 sentences of 0, 1, 7, 40 and max_len = 48 tokens over a vocabulary of 32 and an order-3 model that has a state with 12 arcs
(the binary search takes several trips), steps that back off twice, and tokens without a unigram.  One sentence holds ids outside the
vocabulary, which are clamped."""
import importlib

import numpy as np
import pytest

import lm_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V, MAXLEN = 32, 48
LENS = (0, 1, 7, 40, MAXLEN)


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def model_ngrams(with_eos=True):
    rng = np.random.default_rng(77)
    grams = {tuple(g): (p, b) for g, p, b in R.random_ngrams(rng, V, 3, [150, 200], with_eos=with_eos, missing=(30, 31))}
    for w in range(2, 14):                                           # the state of (5): twelve arcs
        grams.setdefault((5, w), (-0.5 - 0.01 * w, -0.3))
    grams[(5, 6, 7)] = (-0.2, 0.0)                                   # (5, 6) is a state: (5, 6) then 29 backs off twice
    for k in [g for g in grams if g[-1] == 29 and len(g) > 1]:
        del grams[k]
    return [(g, p, b) for g, (p, b) in grams.items() if len(g) == 1 or g[:-1] in grams]


def sentences():
    rng = np.random.default_rng(4)
    rows = np.full((len(LENS), MAXLEN), -9, np.int32)                # what lies behind a sentence is never read
    for b, n in enumerate(LENS):
        rows[b, :n] = rng.integers(0, V, size=n)
    rows[2, :7] = [5, 6, 29, 5, 13, 30, 5]                           # two back-offs at 29, the widest state, a token with no unigram
    rows[3, 3], rows[3, 9], rows[3, 20] = 1000, -5, V                # clamped to 31, 0, 31
    return rows


def backoffs(lm, state, label):
    n = 0
    while state != 0:
        lo, hi = lm.arc_begin[state], lm.arc_begin[state + 1]
        if label in lm.arc_label[lo:hi]:
            break
        state, n = int(lm.backoff_state[state]), n + 1
    return n


@pytest.mark.parametrize("with_eos", [True, False])
def test_equal_to_the_restatement_bit_for_bit(ops, pkg, with_eos):
    grams = model_ngrams(with_eos)
    lm = R.Lm(grams, V, scale=0.7, token_bonus=0.15, oov_log10=-6.5)
    # the model is what the docstring says it is
    s5 = int(lm.uni_next[5])
    assert lm.order == 3 and lm.arc_begin[s5 + 1] - lm.arc_begin[s5] >= 9 and lm.uni_next[30] == 0
    s56 = R.step(lm, s5, 6)[0]
    assert backoffs(lm, s56, 29) == 2
    g = pkg.LmGraph.from_ngrams(grams, V, scale=0.7, token_bonus=0.15, oov_log10=-6.5)
    rows = sentences()
    tok_w, eos_w, total = ops.lm_score(torch.from_numpy(rows).cuda(), torch.tensor(LENS, dtype=torch.int32).cuda(), g)
    torch.cuda.synchronize()
    tok_w, eos_w, total = tok_w.cpu().numpy(), eos_w.cpu().numpy(), total.cpu().numpy()
    bits = lambda x: np.asarray(x, np.float32).view(np.uint32)
    for b, n in enumerate(LENS):
        w_tok, w_eos, w_total = R.score_sentence(lm, rows[b, :n], MAXLEN)
        assert np.array_equal(bits(tok_w[b]), bits(w_tok)), (b, tok_w[b], w_tok)
        assert bits(eos_w[b]) == bits(w_eos) and bits(total[b]) == bits(w_total), (b, eos_w[b], w_eos, total[b], w_total)
        assert (w_eos != 0) == with_eos
    assert total[0] == eos_w[0]                                      # the empty sentence: </s> after <s>, or nothing


def test_lengths_are_clamped_and_refusals(ops, pkg):
    grams = model_ngrams()
    lm, g = R.Lm(grams, V), pkg.LmGraph.from_ngrams(grams, V)
    rows = sentences()[:2, :5].copy()
    rows[:, :] = [[1, 2, 3, 4, 5], [5, 6, 7, 8, 9]]
    tok_w, eos_w, total = ops.lm_score(torch.from_numpy(rows).cuda(), torch.tensor([-3, 99], dtype=torch.int32).cuda(), g)
    torch.cuda.synchronize()
    assert (tok_w[0].cpu().numpy() == 0).all() and total[0].item() == R.score_sentence(lm, [])[2]
    assert total[1].item() == R.score_sentence(lm, rows[1])[2]
    with pytest.raises(pkg.PfhipError):
        ops.lm_score(torch.from_numpy(rows), torch.tensor([1, 1], dtype=torch.int32).cuda(), g)      # a host tensor
