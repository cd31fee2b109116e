"""CPU: the entry points of the top-k CTC head, the prefix beam search and the context graph are exported and bound, and what they
refuse is refused before any HIP call (no device here); both headers still compile as C and as C++ with the new declarations."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPH_SYMBOLS = ["pfhip_ctx_graph_create", "pfhip_ctx_graph_destroy", "pfhip_ctx_graph_vocab", "pfhip_ctx_graph_dump"]
OP_SYMBOLS = ["pfhip_op_ctc_head_topk", "pfhip_op_ctc_head_topk_workspace_bytes", "pfhip_op_ctc_prefix_beam",
              "pfhip_op_ctc_prefix_beam_workspace_bytes"]
INVALID = 1                                     # hipErrorInvalidValue, and PFHIP_ERR_ARG


@pytest.fixture(scope="module")
def lib(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg.load_lib()


@pytest.fixture(scope="module")
def ops_lib(pkg, lib):
    import importlib
    pytest.importorskip("torch")
    return importlib.import_module("asr_2pass_amd.ops")._lib()


def test_symbols_are_exported_and_bound(pkg, lib, ops_lib):
    for name in GRAPH_SYMBOLS:
        assert hasattr(lib, name) and name in pkg.ABI_SYMBOLS, name
    for name in OP_SYMBOLS:
        assert hasattr(lib, name), name
    assert len(ops_lib.pfhip_op_ctc_head_topk.argtypes) == 18 and len(ops_lib.pfhip_op_ctc_prefix_beam.argtypes) == 23
    assert hasattr(pkg, "ContextGraph")


def test_workspace_sizes(ops_lib):
    head, topk = ops_lib.pfhip_op_ctc_head_workspace_bytes, ops_lib.pfhip_op_ctc_head_topk_workspace_bytes
    # per row and 128-column tile: the greedy triple plus k (value, column) pairs
    assert topk(200, 300, 10) == head(200, 300) + 2 * 3 * 10 * 200 * 4
    assert topk(200, 300, 0) == 0 and topk(200, 300, 17) == 0
    beam = ops_lib.pfhip_op_ctc_prefix_beam_workspace_bytes
    assert beam(337, 3, 5, None) == 2 * 4 * 337 * 5             # a (parent, token) node per row and beam slot
    assert beam(-1, 3, 5, None) == 0 and beam(337, 3, 0, None) == 0


def test_refused_without_a_device(pkg, ops_lib):
    f = ops_lib.pfhip_op_ctc_head_topk
    one = ctypes.c_void_p(64)                   # never dereferenced: every call below is refused by its argument checks
    for k, V in ((0, 300), (17, 300), (5, 4)):
        assert f(one, 32, one, 32, one, 1.0, 8, V, 32, k, one, one, one, one, one, one, 1 << 30, None) == INVALID
    assert f(one, 32, one, 32, one, 1.0, 8, 300, 32, 4, one, one, one, None, one, one, 1 << 30, None) == INVALID       # no topk_ids
    assert f(one, 32, one, 32, one, 1.0, 8, 300, 32, 4, one, one, one, one, one, one, 16, None) == INVALID             # short workspace
    b = ops_lib.pfhip_op_ctc_prefix_beam

    def beam(k=4, rows=10, B=1, V=50, blank=0, fb=3, sb=3, graph=None, nbest=3, ws=one, nbytes=1 << 20, n_hyp=one):
        return b(one, one, k, rows, one, one, B, V, blank, fb, sb, graph, nbest, 8, n_hyp, one, one, one, one, one, ws, nbytes, None)

    for bad in (dict(k=0), dict(k=17), dict(fb=0), dict(fb=5), dict(sb=0), dict(sb=17), dict(nbest=0), dict(nbest=4), dict(blank=50),
                dict(blank=-1), dict(V=0), dict(rows=-1), dict(B=-1), dict(ws=None), dict(nbytes=8), dict(n_hyp=None)):
        assert beam(**bad) == INVALID, bad
    g = pkg.ContextGraph([[1, 2]], [1.0], 49)
    assert beam(graph=g.handle) == INVALID      # a graph built for another vocabulary
    assert pkg.load_lib().pfhip_ctx_graph_vocab(g.handle) == 49
    assert pkg.load_lib().pfhip_ctx_graph_create(None, None, None, 1, 10, None) == INVALID


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_headers_compile(tmp_path, lang):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if cc is None:
        pytest.fail("no compiler to check the headers with")
    src = tmp_path / ("h.c" if lang == "c" else "h.cpp")
    src.write_text('#include "pfhip.h"\n#include "pfhip_ops.h"\n'
                   "int main(void) { pfhip_ctx_graph* g = 0; return pfhip_op_ctc_prefix_beam_workspace_bytes(0, 0, 1, g) != 0; }\n")
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
