"""CPU: the search over a non-autoregressive head's candidates (pfhip_op_nbest_ctx_beam) is exported and bound, and what the entry
refuses is refused before any device pointer is touched (no device here: every pointer below is the address 64 and must never be
read)."""
import ctypes
import importlib
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                                     # hipErrorInvalidValue


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


def test_symbols_are_exported_and_bound(pkg, lib, ops_lib):
    for name in ("pfhip_op_nbest_ctx_beam", "pfhip_op_nbest_ctx_beam_workspace_bytes"):
        assert hasattr(lib, name), name
    for name in ("pfhip_offline_forward_bias", "pfhip_offline_forward_bias_s16"):
        assert hasattr(lib, name) and name in pkg.ABI_SYMBOLS, name
    assert len(lib.pfhip_offline_forward_bias.argtypes) == 15 and hasattr(pkg.ParaformerHip, "forward_bias")
    assert len(ops_lib.pfhip_op_nbest_ctx_beam.argtypes) == 24
    assert hasattr(importlib.import_module("asr_2pass_amd.ops"), "nbest_ctx_beam")


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_workspace_sizes(pkg, ops_lib):
    size = ops_lib.pfhip_op_nbest_ctx_beam_workspace_bytes
    g = pkg.ContextGraph([[1, 2]], [1.0], 50)
    image = (ops_lib.pfhip_op_ctc_prefix_beam_workspace_bytes(10, 1, 1, g.handle) - ops_lib.pfhip_op_ctc_prefix_beam_workspace_bytes(10, 1, 1, None))
    hs = (ctypes.c_void_p * 1)(g.handle)
    # descriptors 16 B an utterance | a 48-byte table entry a graph | the graph's image | a (parent, token) node per row and slot of
    # the LARGEST beam
    assert size(337, 3, 8, ints(3, 1, 8), ints(5, 16, 7), ints(1, 9, 2), ints(-1, -1, -1), None, 0) == 48 + 2 * 4 * 337 * 16
    assert size(337, 3, 8, ints(3, 1, 8), ints(5, 9, 7), ints(1, 9, 2), ints(0, -1, 0), hs, 1) == 48 + 48 + image + 2 * 4 * 337 * 9
    assert size(337, 3, 8, ints(3, 0, 8), ints(5, 16, 7), ints(1, 9, 2), ints(-1, -1, -1), None, 0) == 0      # width 0
    assert size(337, 3, 7, ints(3, 1, 8), ints(5, 16, 7), ints(1, 9, 2), ints(-1, -1, -1), None, 0) == 0      # width above k
    assert size(-1, 3, 8, ints(3, 1, 8), ints(5, 16, 7), ints(1, 9, 2), ints(-1, -1, -1), None, 0) == 0


def test_bad_arguments_are_refused_without_a_device(pkg, ops_lib):
    f = ops_lib.pfhip_op_nbest_ctx_beam
    one = ctypes.c_void_p(64)
    g50, g49 = pkg.ContextGraph([[1, 2]], [1.0], 50), pkg.ContextGraph([[1, 2]], [1.0], 49)
    names = ("cand_ids", "cand_logp", "row_off", "length", "n_hyp", "ids", "n_tokens", "score", "am_score", "ctx_score")

    def call(wd=(3, 1, 8), bm=(5, 1, 16), nb=(2, 1, 4), go=(0, -1, -1), graphs=(g50,), k=8, rows=40, B=3, V=50, ws=one, nbytes=1 << 20,
             max_tokens=8, null=None):
        hs = (ctypes.c_void_p * max(len(graphs), 1))(*[None if h is None else h.handle for h in graphs])
        p = {n: (None if n == null else one) for n in names}
        return f(p["cand_ids"], p["cand_logp"], k, rows, p["row_off"], p["length"], B, V, ints(*wd), ints(*bm), ints(*nb), ints(*go), hs,
                 len(graphs), max_tokens, p["n_hyp"], p["ids"], p["n_tokens"], p["score"], p["am_score"], p["ctx_score"], ws, nbytes, None)

    bad = [dict(wd=(9, 1, 8), k=9), dict(wd=(3, 0, 8)), dict(wd=(-1, 1, 8)), dict(wd=(3, 1, 8), k=7), dict(bm=(17, 1, 16)), dict(bm=(0, 1, 16)),
           dict(bm=(-1, 1, 16)), dict(nb=(0, 1, 4)), dict(nb=(6, 1, 4)), dict(nb=(2, 1, 17)), dict(go=(1, -1, -1)), dict(go=(0, -2, -1)),
           dict(go=(0, -1, 0), graphs=(g50, g49)), dict(go=(0, -1, 1), graphs=(g50, g49)), dict(graphs=(None,)), dict(V=49), dict(k=0),
           dict(k=9), dict(V=0, go=(-1, -1, -1), graphs=()), dict(rows=-1), dict(B=-1), dict(B=65536), dict(max_tokens=-1), dict(ws=None),
           dict(nbytes=8), dict(nbytes=48 + 48 + 64)]
    bad += [dict(null=n) for n in names]
    for kw in bad:
        assert call(**kw) == INVALID, kw


def test_the_model_call_refuses_a_null_handle(lib):
    """PFHIP_ERR_ARG before anything else is looked at."""
    assert lib.pfhip_offline_forward_bias(None, None, None, 0, 0, None, None, 0, None, None, None, None, 0, None, None) == 1
    assert lib.pfhip_offline_forward_bias_s16(None, None, None, 0, 0, None, None, 0, None, None, None, None, 0, None, None) == 1


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles(tmp_path, lang):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if cc is None:
        pytest.fail("no compiler to check the headers with")
    src = tmp_path / ("h.c" if lang == "c" else "h.cpp")
    src.write_text('#include "pfhip.h"\n#include "pfhip_ops.h"\n'
                   "int main(void) { pfhip_bias_opts s; pfhip_bias_out o; s.graph = 0; o.max_tokens = 0; (void)s; (void)o;\n"
                   "  if (pfhip_offline_forward_bias(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, &s, 1, 0, &o) == PFHIP_OK) return 1;\n"
                   "  return pfhip_op_nbest_ctx_beam_workspace_bytes(0, 0, 1, 0, 0, 0, 0, 0, 0) != 0\n"
                   "      || pfhip_op_nbest_ctx_beam(0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == 0; }\n")
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
