"""CPU: the builder of the token n-gram language model (csrc/lm_graph.cpp through LmGraph) against the plain-Python restatement
tests/lm_ref.py — the dump must be equal BIT FOR BIT — and the ARPA reader against from_ngrams, with everything it must refuse.  No
device is touched.  The ARPA texts are written here."""
import os

import numpy as np
import pytest

import lm_ref as R

V = 12
EOS, BOS, UNK = V, V + 1, V + 2
NAMES = ["t%d" % i for i in range(V)]


@pytest.fixture(scope="module")
def LmGraph(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    pkg.load_lib()
    return pkg.LmGraph


def same(got, want):
    """The names of the dump's entries that differ (floats by their bits)."""
    bad = []
    for k, w in want.items():
        g, w = np.asarray(got[k]), np.asarray(w)
        eq = g.shape == w.shape and (np.array_equal(g.view(np.uint32), w.view(np.uint32)) if w.dtype == np.float32 else np.array_equal(g, w))
        if not eq:
            bad.append(k)
    return bad


def both(LmGraph, grams, vocab=V, **kw):
    g = LmGraph.from_ngrams(grams, vocab, **kw)
    r = R.Lm(grams, vocab, **kw)
    assert g.order == r.order
    d = g.dump()
    assert same(d, r.dump()) == [], (same(d, r.dump()), d, r.dump())
    return d, r


UNI = [((0,), -1.0, -0.5), ((1,), -0.7, -0.25), ((2,), -1.3, -0.125), ((EOS,), -1.1, 0.0), ((BOS,), -99.0, -0.4)]
BI = [((BOS, 0), -0.3, -0.2), ((0, 1), -0.4, -0.3), ((1, 2), -0.6, -0.1), ((1, EOS), -0.2, 0.0), ((0, 0), -0.9, 0.0)]
TRI = [((BOS, 0, 1), -0.11, 0.0), ((0, 1, 2), -0.21, 0.0), ((0, 1, EOS), -0.31, 0.0)]


def test_unigrams_alone(LmGraph):
    d, _ = both(LmGraph, UNI, scale=0.7, token_bonus=0.3)
    assert d["arc_begin"].tolist() == [0, 0] and d["start"] == 0 and d["has_eos"] == 1 and d["uni_next"].tolist() == [0] * (V + 1)
    # the weight rule, spelled out once: a token takes the bonus, </s> does not, a token without a unigram scores oov_log10
    s, b = float(np.float32(0.7)), float(np.float32(0.3))
    assert d["uni_w"][0] == np.float32(-1.0 * R.LN10 * s + b) and d["uni_w"][V] == np.float32(-1.1 * R.LN10 * s)
    assert d["uni_w"][5] == np.float32(-10.0 * R.LN10 * s + b)


def test_bigrams(LmGraph):
    d, _ = both(LmGraph, UNI + BI, scale=0.5, token_bonus=0.1)
    # states: 0, then (0), (1), (2), (</s>), (<s>) by label
    assert d["start"] == 5 and d["uni_next"][:3].tolist() == [1, 2, 3] and d["uni_next"][V] == 4
    assert d["arc_begin"].tolist() == [0, 0, 2, 4, 4, 4, 5]
    assert d["arc_label"].tolist() == [0, 1, 2, EOS, 0] and d["arc_next"].tolist() == [1, 2, 3, 4, 1]
    assert d["backoff_state"].tolist() == [0] * 6
    assert d["backoff_w"][1] == np.float32(-0.5 * R.LN10 * float(np.float32(0.5))) and d["backoff_w"][0] == 0


def test_trigrams(LmGraph):
    d, _ = both(LmGraph, UNI + BI + TRI)
    # the state of (0, 1) falls back to the state of (1); the arc (0, 1) -> 2 lands in the state of (1, 2)
    S1 = 1 + len(UNI)                                                # the first state of length 2
    two = sorted(g[0] for g in BI)
    st = {g: S1 + i for i, g in enumerate(two)}
    assert d["backoff_state"][st[(0, 1)]] == 2 and d["backoff_state"][st[(BOS, 0)]] == 1
    a = d["arc_begin"][st[(0, 1)]]
    assert d["arc_label"][a:d["arc_begin"][st[(0, 1)] + 1]].tolist() == [2, EOS]
    assert d["arc_next"][a] == st[(1, 2)] and d["arc_next"][a + 1] == st[(1, EOS)]


def test_a_history_whose_suffix_is_no_state_and_a_token_without_a_unigram(LmGraph):
    """Token 3 has no unigram, so (0, 3) is a state whose suffix (3) is none: it falls back to state 0, and the arc into it from
    state (0) exists while state 0 sends token 3 to itself."""
    grams = UNI + BI + [((0, 3), -0.5, -0.7), ((0, 3, 1), -0.2, 0.0)]
    d, r = both(LmGraph, grams)
    two = sorted(g[0] for g in BI + [((0, 3), 0, 0)])
    s03 = 1 + len(UNI) + two.index((0, 3))
    assert d["backoff_state"][s03] == 0 and d["uni_next"][3] == 0 and d["uni_w"][3] == np.float32(-10.0 * R.LN10)
    assert R.step(r, 1, 3)[0] == s03 and R.step(r, s03, 1)[1] == np.float32(-0.2 * R.LN10)


def test_an_ngram_predicting_bos_is_dropped(LmGraph):
    d0, _ = both(LmGraph, UNI + BI)
    d1, _ = both(LmGraph, UNI + BI + [((0, BOS), -0.5, -0.1)], order=2)
    assert same(d1, d0) == []


def test_unk_present_and_absent(LmGraph):
    d0, _ = both(LmGraph, UNI + BI, oov_log10=-7.5)
    d1, _ = both(LmGraph, UNI + BI + [((UNK,), -4.25, 0.0)], oov_log10=-7.5, token_bonus=0.5)
    assert d0["uni_w"][7] == np.float32(-7.5 * R.LN10) and d1["uni_w"][7] == np.float32(-4.25 * R.LN10 + 0.5)
    assert len(d1["backoff_w"]) == len(d0["backoff_w"])             # <unk> is no state


def test_missing_bos_and_missing_eos(LmGraph):
    grams = [g for g in UNI + BI + TRI if BOS not in g[0]]
    d, _ = both(LmGraph, grams)
    assert d["start"] == 0 and d["has_eos"] == 1
    grams = [g for g in UNI + BI + TRI if EOS not in g[0]]
    d, _ = both(LmGraph, grams)
    assert d["has_eos"] == 0 and d["start"] > 0


@pytest.mark.parametrize("seed", range(6))
def test_random_sets_up_to_order_4(LmGraph, seed):
    rng = np.random.default_rng(100 + seed)
    order = 2 + seed % 3
    grams = R.random_ngrams(rng, V, order, [30, 40, 40][:order - 1], with_bos=seed != 1, with_eos=seed != 2, with_unk=seed % 2 == 0,
                            missing=(4, 9) if seed >= 3 else ())
    rng.shuffle(grams)
    both(LmGraph, [tuple(g) for g in grams], scale=0.3 + 0.1 * seed, token_bonus=0.25 * seed, oov_log10=-6.0)


def test_create_refuses(LmGraph, pkg):
    def bad(grams, text, **kw):
        with pytest.raises(pkg.PfhipError) as e:
            LmGraph.from_ngrams(grams, V, **kw)
        assert e.value.status == 1 and text in str(e.value), str(e.value)

    bad(UNI, "order", order=7)
    bad(UNI + [((0, V + 3), -1.0, 0.0)], "label")
    bad(UNI + [((-1,), -1.0, 0.0)], "label")
    bad(UNI + [((0, UNK), -1.0, 0.0)], "<unk>")
    bad(UNI + [((0,), -2.0, 0.0)], "twice")
    bad(UNI + [((3,), float("nan"), 0.0)], "non-finite")
    bad(UNI + [((3,), -1.0, float("inf"))], "non-finite")
    bad(UNI, "finite", scale=float("inf"))
    bad(UNI + [((3,), -2e38, 0.0)], "fp32")                       # finite in double, beyond FLT_MAX once times ln 10


# ---- the ARPA reader ----------------------------------------------------------------------------------------------------------------
def write(tmp_path, text, name="lm.arpa"):
    p = tmp_path / name
    p.write_bytes(text if isinstance(text, bytes) else text.encode("utf-8"))
    return str(p)


@pytest.mark.parametrize("seed", range(3))
def test_arpa_gives_the_graph_of_from_ngrams(LmGraph, tmp_path, seed):
    rng = np.random.default_rng(7 + seed)
    grams = R.random_ngrams(rng, V, 2 + seed, [25, 30, 30][:1 + seed], with_unk=seed == 1)
    g = LmGraph.from_arpa(write(tmp_path, R.arpa_text(grams, NAMES, V)), NAMES, scale=0.6, token_bonus=0.2, oov_log10=-8.0)
    want = LmGraph.from_ngrams(grams, V, scale=0.6, token_bonus=0.2, oov_log10=-8.0)
    assert g.n_skipped == 0 and g.order == want.order and same(g.dump(), want.dump()) == []
    assert same(g.dump(), R.Lm(grams, V, scale=0.6, token_bonus=0.2, oov_log10=-8.0).dump()) == []


def test_arpa_words_are_matched_byte_for_byte_and_skips_are_counted(LmGraph, tmp_path):
    names = ["的", "▁the", "a", "a", "<s>"] + NAMES[5:]                # a duplicate: the lowest id wins; "<s>" as a token never matches
    text = ("\\data\\\nngram 1=6\nngram 2=4\n\n\\1-grams:\n-1.0\t的\t-0.5\n-0.7 ▁the -0.25\r\n-1.3\ta\t-0.1\n-2.0\tthe\n-99\t<s>\t-0.4\n"
            "-1.1\t</s>\n\n\\2-grams:\n-0.3\t<s> 的\n-0.4\t的 a\n-0.5\t的 A\n-0.6\t<unk> a\n\n\\end\\\n")
    g = LmGraph.from_arpa(write(tmp_path, text), names)
    assert g.n_skipped == 3                                          # "the", "的 A", "<unk> a"
    grams = [((0,), -1.0, -0.5), ((1,), -0.7, -0.25), ((2,), -1.3, -0.1), ((BOS,), -99.0, -0.4), ((EOS,), -1.1, 0.0),
             ((BOS, 0), -0.3, 0.0), ((0, 2), -0.4, 0.0)]
    assert same(g.dump(), R.Lm(grams, V).dump()) == []


HEAD = "\\data\\\nngram 1=2\nngram 2=1\n\n"
BODY = "\\1-grams:\n-1.0\tt0\t-0.5\n-0.7\tt1\t-0.2\n\n\\2-grams:\n-0.3\tt0 t1\n\n"
REFUSED = {
    "no data line": (BODY + "\\end\\\n", "\\data\\"),
    "no end line": (HEAD + BODY, "\\end\\"),
    "truncated in a section": (HEAD + "\\1-grams:\n-1.0\tt0\t-0.5\n", "count"),
    "count above its section": ("\\data\\\nngram 1=3\nngram 2=1\n\n" + BODY + "\\end\\\n", "count"),
    "count below its section": ("\\data\\\nngram 1=1\nngram 2=1\n\n" + BODY + "\\end\\\n", "count"),
    "a section missing": (HEAD + "\\1-grams:\n-1.0\tt0\t-0.5\n-0.7\tt1\t-0.2\n\n\\end\\\n", "expected \\2-grams:"),
    "too few fields": (HEAD + BODY.replace("-0.3\tt0 t1", "-0.3\tt0") + "\\end\\\n", "fields"),
    "too many fields": (HEAD + BODY.replace("-0.7\tt1\t-0.2", "-0.7\tt1\t-0.2\t7") + "\\end\\\n", "fields"),
    "nan": (HEAD + BODY.replace("-0.7", "nan") + "\\end\\\n", "finite"),
    "inf back-off": (HEAD + BODY.replace("-0.2", "-inf") + "\\end\\\n", "finite"),
    "overflowing number": (HEAD + BODY.replace("-0.7", "-1e999") + "\\end\\\n", "finite"),
    "not a number": (HEAD + BODY.replace("-0.7", "-0.7x") + "\\end\\\n", "finite"),
    "order above the cap": ("\\data\\\n" + "".join("ngram %d=0\n" % n for n in range(1, 8)) + "\n\\end\\\n", "order above"),
    "orders out of turn": ("\\data\\\nngram 2=1\n\n\\end\\\n", "in turn"),
    "negative count": ("\\data\\\nngram 1=-2\n\n\\1-grams:\n\\end\\\n", "negative"),
    "count beyond int32": ("\\data\\\nngram 1=4000000000\n\n\\1-grams:\n\\end\\\n", "int32"),
    "counts whose product is beyond int32": ("\\data\\\nngram 1=2\nngram 2=2\nngram 3=400000000\n\n\\1-grams:\n\\end\\\n", "int32"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_arpa_refusals(LmGraph, pkg, tmp_path, case):
    text, say = REFUSED[case]
    with pytest.raises(pkg.PfhipError) as e:
        LmGraph.from_arpa(write(tmp_path, text), NAMES)
    assert e.value.status == 1 and say in str(e.value), str(e.value)


def test_arpa_good_file_and_missing_file(LmGraph, pkg, tmp_path):
    g = LmGraph.from_arpa(write(tmp_path, HEAD + BODY + "\\end\\\n"), NAMES)
    assert g.order == 2 and g.dump()["arc_label"].tolist() == [1]
    with pytest.raises(pkg.PfhipError) as e:
        LmGraph.from_arpa(str(tmp_path / "none.arpa"), NAMES)
    assert "cannot open" in str(e.value)


def test_dump_capacity(LmGraph, pkg):
    import ctypes
    g = LmGraph.from_ngrams(UNI + BI, V)
    lib = pkg.load_lib()
    ci = ctypes.c_int
    n = [ci() for _ in range(4)]
    f, i = (ctypes.c_float * 64)(), (ctypes.c_int32 * 64)()
    args = lambda cu, cs, ca: (g.handle, *[ctypes.byref(x) for x in n], f, i, cu, i, f, i, cs, i, i, f, ca)
    assert lib.pfhip_lm_graph_dump(*args(V + 1, 6, 5)) == 0
    assert [x.value for x in n] == [6, 5, 5, 1]
    for caps in ((V, 6, 5), (V + 1, 5, 5), (V + 1, 6, 4)):
        assert lib.pfhip_lm_graph_dump(*args(*caps)) == 5            # PFHIP_ERR_CAPACITY
    assert lib.pfhip_lm_graph_dump(g.handle, *[ctypes.byref(x) for x in n], f, None, V + 1, i, f, i, 6, i, i, f, 5) == 1
    assert lib.pfhip_lm_graph_vocab(g.handle) == V and lib.pfhip_lm_graph_vocab(None) == 0 and lib.pfhip_lm_graph_order(None) == 0
