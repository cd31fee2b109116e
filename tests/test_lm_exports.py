"""CPU: the token n-gram language model's entries are exported and bound, what the operator entries refuse is refused before any
device pointer is touched (no device here: every pointer below is the address 64 and must never be read), the headers compile as
C and as C++, and the ARPA reader survives its list of damaged texts under the address and undefined-behaviour sanitizers (a
stand-alone program: tools/fuzz/lm_arpa_fuzz.cpp linked with csrc/lm_graph.cpp alone)."""
import ctypes
import importlib
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                                     # hipErrorInvalidValue
V = 50
GRAMS = [((0,), -1.0, -0.5), ((1,), -0.7, -0.2), ((V,), -1.1, 0.0), ((V + 1,), -99.0, -0.3), ((V + 1, 0), -0.3, 0.0), ((0, 1), -0.4, 0.0)]


@pytest.fixture(scope="module")
def lib(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg.load_lib()


@pytest.fixture(scope="module")
def ops_lib(pkg, lib):
    pytest.importorskip("torch")
    return importlib.import_module("asr_2pass_amd.ops")._lib()


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_symbols_are_exported_and_bound(pkg, lib, ops_lib):
    for name in ("pfhip_lm_graph_create", "pfhip_lm_graph_create_from_arpa", "pfhip_lm_graph_destroy", "pfhip_lm_graph_vocab",
                 "pfhip_lm_graph_order", "pfhip_lm_graph_dump"):
        assert hasattr(lib, name) and name in pkg.ABI_SYMBOLS, name
    for name in ("pfhip_op_lm_score", "pfhip_op_lm_score_workspace_bytes", "pfhip_op_nbest_ctx_beam_lm", "pfhip_op_nbest_ctx_beam_lm_workspace_bytes",
                 "pfhip_op_ctc_prefix_beam_multi_lm", "pfhip_op_ctc_prefix_beam_multi_lm_workspace_bytes"):
        assert hasattr(lib, name), name
    # the siblings' arguments plus the model and the lm_score output
    assert len(ops_lib.pfhip_op_nbest_ctx_beam_lm.argtypes) == len(ops_lib.pfhip_op_nbest_ctx_beam.argtypes) + 2 == 26
    assert len(ops_lib.pfhip_op_ctc_prefix_beam_multi_lm.argtypes) == len(ops_lib.pfhip_op_ctc_prefix_beam_multi.argtypes) + 2 == 27
    assert len(ops_lib.pfhip_op_lm_score.argtypes) == 11
    ops = importlib.import_module("asr_2pass_amd.ops")
    assert all(hasattr(ops, n) for n in ("lm_score", "nbest_ctx_beam_lm", "ctc_prefix_beam_multi_lm"))
    assert all(hasattr(pkg.LmGraph, n) for n in ("from_arpa", "from_ngrams", "dump"))


def test_workspace_sizes(pkg, ops_lib):
    lm = pkg.LmGraph.from_ngrams(GRAMS, V)
    d = lm.dump()
    S, A = len(d["backoff_w"]), len(d["arc_label"])
    image = (4 * (2 * (V + 1) + (S + 1) + 2 * S + 3 * A) + 15) // 16 * 16
    assert ops_lib.pfhip_op_lm_score_workspace_bytes(lm.handle) == image and ops_lib.pfhip_op_lm_score_workspace_bytes(None) == 0
    g = pkg.ContextGraph([[1, 2]], [1.0], V)
    hs = (ctypes.c_void_p * 1)(g.handle)
    args = (337, 3, 8, ints(3, 1, 8), ints(5, 9, 7), ints(1, 9, 2), ints(0, -1, 0), hs, 1)
    plain = ops_lib.pfhip_op_nbest_ctx_beam_workspace_bytes(*args)
    assert plain > 0 and ops_lib.pfhip_op_nbest_ctx_beam_lm_workspace_bytes(*args, lm.handle) == plain + image
    assert ops_lib.pfhip_op_nbest_ctx_beam_lm_workspace_bytes(*args, None) == plain
    plain = ops_lib.pfhip_op_ctc_prefix_beam_multi_workspace_bytes(*args)
    assert plain > 0 and ops_lib.pfhip_op_ctc_prefix_beam_multi_lm_workspace_bytes(*args, lm.handle) == plain + image
    bad = (337, 3, 8, ints(3, 0, 8), ints(5, 9, 7), ints(1, 9, 2), ints(0, -1, 0), hs, 1)                      # width 0
    assert ops_lib.pfhip_op_nbest_ctx_beam_lm_workspace_bytes(*bad, lm.handle) == 0


def test_lm_score_refuses_without_a_device(pkg, ops_lib):
    f = ops_lib.pfhip_op_lm_score
    one = ctypes.c_void_p(64)
    lm = pkg.LmGraph.from_ngrams(GRAMS, V)

    def call(ids=one, length=one, B=2, max_len=5, h=lm.handle, tok_w=one, eos_w=one, total=one, ws=one, nbytes=1 << 20):
        return f(ids, length, B, max_len, h, tok_w, eos_w, total, ws, nbytes, None)

    for kw in (dict(h=None), dict(B=-1), dict(max_len=-1), dict(ws=None), dict(nbytes=8), dict(ids=None), dict(length=None), dict(tok_w=None),
               dict(eos_w=None), dict(total=None), dict(B=1 << 20, max_len=1 << 12)):
        assert call(**kw) == INVALID, kw


def test_the_searches_refuse_without_a_device(pkg, ops_lib):
    one = ctypes.c_void_p(64)
    lm, lm49 = pkg.LmGraph.from_ngrams(GRAMS, V), pkg.LmGraph.from_ngrams(GRAMS[:2], V - 1)
    g50 = pkg.ContextGraph([[1, 2]], [1.0], V)
    names = ("cand_ids", "cand_logp", "row_off", "length", "n_hyp", "ids", "n_tokens", "score", "am_score", "ctx_score", "lm_score")

    def call(entry, wd=(3, 1, 8), bm=(5, 1, 16), nb=(2, 1, 4), go=(0, -1, -1), k=8, rows=40, B=3, Vv=V, h=lm.handle, ws=one, nbytes=1 << 20,
             max_tokens=8, null=None):
        hs = (ctypes.c_void_p * 1)(g50.handle)
        p = {n: (None if n == null else one) for n in names}
        head = (p["cand_ids"], p["cand_logp"], k, rows, p["row_off"], p["length"], B, Vv)
        tail = (ints(*wd), ints(*bm), ints(*nb), ints(*go), hs, 1, h, max_tokens, p["n_hyp"], p["ids"], p["n_tokens"], p["score"], p["am_score"],
                p["ctx_score"], p["lm_score"], ws, nbytes, None)
        if entry == "nar":
            return ops_lib.pfhip_op_nbest_ctx_beam_lm(*head, *tail)
        return ops_lib.pfhip_op_ctc_prefix_beam_multi_lm(*head, 0, *tail)                                     # blank 0

    bad = [dict(h=lm49.handle), dict(wd=(9, 1, 8)), dict(wd=(-1, 1, 8)), dict(bm=(17, 1, 16)), dict(nb=(6, 1, 4)), dict(go=(1, -1, -1)), dict(Vv=49),
           dict(k=0), dict(rows=-1), dict(B=-1), dict(B=65536), dict(max_tokens=-1), dict(ws=None), dict(nbytes=8)]
    bad += [dict(null=n) for n in names]
    for entry in ("nar", "ctc"):
        for kw in bad:
            assert call(entry, **kw) == INVALID, (entry, kw)
        # without a model the sibling's refusals hold, and lm_score is still needed
        for kw in (dict(h=None, wd=(9, 1, 8)), dict(h=None, null="lm_score"), dict(h=None, nbytes=8), dict(h=None, null="score")):
            assert call(entry, **kw) == INVALID, (entry, kw)
    assert call("nar", wd=(3, 0, 8)) == INVALID                      # width 0 (in the CTC search first_beam 0 means "no search")


def test_graph_entries_refuse_null_arguments(lib):
    h = ctypes.c_void_p()
    assert lib.pfhip_lm_graph_create(1, None, None, None, None, 5, 1.0, 0.0, -5.0, ctypes.byref(h)) == 1
    assert b"counts" in lib.pfhip_last_error()
    assert lib.pfhip_lm_graph_create(1, ints(0), None, None, None, 5, 1.0, 0.0, -5.0, None) == 1
    assert lib.pfhip_lm_graph_create(1, ints(1), None, None, None, 5, 1.0, 0.0, -5.0, ctypes.byref(h)) == 1 and not h.value
    assert lib.pfhip_lm_graph_create(1, ints(0), None, None, None, 0, 1.0, 0.0, -5.0, ctypes.byref(h)) == 1
    assert lib.pfhip_lm_graph_create(1, ints(0), None, None, None, 5, 1.0, 0.0, -5.0, ctypes.byref(h)) == 0 and h.value      # no n-gram at all
    assert lib.pfhip_lm_graph_order(h) == 1 and lib.pfhip_lm_graph_vocab(h) == 5
    lib.pfhip_lm_graph_destroy(h)
    lib.pfhip_lm_graph_destroy(None)
    assert lib.pfhip_lm_graph_create_from_arpa(None, None, 5, 1.0, 0.0, -5.0, ctypes.byref(h), None) == 1


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_headers_compile(tmp_path, lang):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if cc is None:
        pytest.fail("no compiler to check the headers with")
    src = tmp_path / ("h.c" if lang == "c" else "h.cpp")
    src.write_text('#include "pfhip.h"\n#include "pfhip_ops.h"\n'
                   "int main(void) { pfhip_lm_graph* g = 0; long long skipped = 0; int n[PFHIP_LM_ORDER_MAX] = {0};\n"
                   "  if (pfhip_lm_graph_create(1, n, 0, 0, 0, 5, 1.0f, 0.0f, -5.0f, &g) != PFHIP_OK) return 1;\n"
                   "  if (pfhip_lm_graph_create_from_arpa(0, 0, 5, 1.0f, 0.0f, -5.0f, &g, &skipped) == PFHIP_OK) return 1;\n"
                   "  if (pfhip_lm_graph_dump(g, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == PFHIP_OK) return 1;\n"
                   "  pfhip_lm_graph_destroy(g);\n"
                   "  return pfhip_lm_graph_vocab(0) + pfhip_lm_graph_order(0) + (int)pfhip_op_lm_score_workspace_bytes(0)\n"
                   "      + (pfhip_op_lm_score(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == 0)\n"
                   "      + (pfhip_op_nbest_ctx_beam_lm_workspace_bytes(0, 0, 1, 0, 0, 0, 0, 0, 0, 0) != 0)\n"
                   "      + (pfhip_op_nbest_ctx_beam_lm(0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == 0)\n"
                   "      + (pfhip_op_ctc_prefix_beam_multi_lm_workspace_bytes(0, 0, 1, 0, 0, 0, 0, 0, 0, 0) != 0)\n"
                   "      + (pfhip_op_ctc_prefix_beam_multi_lm(0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == 0); }\n")
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_arpa_reader_under_the_sanitizers(tmp_path):
    """Host code only, in a program of its own: compiled here with -fsanitize=address,undefined and run over its fixed list of
    damaged ARPA texts (truncated files, huge and negative counts, lines of 10^6 characters, NUL bytes)."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("no g++ to build tools/fuzz/lm_arpa_fuzz.cpp with")
    exe = tmp_path / "lm_arpa_fuzz"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "asr-2pass_amd", "csrc", "lm_graph.cpp"),
           os.path.join(ROOT, "tools", "fuzz", "lm_arpa_fuzz.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "texts behaved" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
