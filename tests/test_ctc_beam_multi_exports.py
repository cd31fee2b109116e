"""CPU: the per-utterance form of the prefix beam search (pfhip_op_ctc_prefix_beam_multi) and the per-utterance sets of the
SenseVoice forward (pfhip_svs_forward_beam_sets) are exported and bound, and what the entries refuse is refused before any device
pointer is touched (no device here: every pointer below is the address 64 and must never be read)."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    for name in ("pfhip_op_ctc_prefix_beam_multi", "pfhip_op_ctc_prefix_beam_multi_workspace_bytes"):
        assert hasattr(lib, name), name
    for name in ("pfhip_svs_forward_beam_sets", "pfhip_svs_forward_beam_sets_s16"):
        assert hasattr(lib, name) and name in pkg.ABI_SYMBOLS, name
    assert len(ops_lib.pfhip_op_ctc_prefix_beam_multi.argtypes) == 25
    import importlib
    assert hasattr(importlib.import_module("asr_2pass_amd.ops"), "ctc_prefix_beam_multi")


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_workspace_sizes(pkg, ops_lib):
    size = ops_lib.pfhip_op_ctc_prefix_beam_multi_workspace_bytes
    g = pkg.ContextGraph([[1, 2]], [1.0], 50)
    image = (ops_lib.pfhip_op_ctc_prefix_beam_workspace_bytes(10, 1, 1, g.handle) - ops_lib.pfhip_op_ctc_prefix_beam_workspace_bytes(10, 1, 1, None))
    hs = (ctypes.c_void_p * 1)(g.handle)
    # descriptors 16 B an utterance | a 48-byte table entry a graph | the graph's image | a (parent, token) node per row and slot of
    # the LARGEST second_beam among the searching utterances
    assert size(337, 3, 10, ints(3, 0, 10), ints(5, 16, 7), ints(1, 9, 2), ints(-1, -1, -1), None, 0) == 48 + 2 * 4 * 337 * 7
    assert size(337, 3, 10, ints(3, 0, 10), ints(5, 16, 7), ints(1, 9, 2), ints(0, -1, 0), hs, 1) == 48 + 48 + image + 2 * 4 * 337 * 7
    assert size(337, 3, 10, ints(3, 0, 11), ints(5, 16, 11), ints(1, 9, 2), ints(-1, -1, -1), None, 0) == 0      # first_beam above k
    assert size(-1, 3, 10, ints(3, 0, 10), ints(5, 16, 7), ints(1, 9, 2), ints(-1, -1, -1), None, 0) == 0


def test_bad_descriptors_are_refused_without_a_device(pkg, ops_lib):
    f = ops_lib.pfhip_op_ctc_prefix_beam_multi
    one = ctypes.c_void_p(64)
    g50, g49 = pkg.ContextGraph([[1, 2]], [1.0], 50), pkg.ContextGraph([[1, 2]], [1.0], 49)

    def call(fb=(3, 0, 10), sb=(5, 0, 10), nb=(2, 0, 4), go=(0, -1, -1), graphs=(g50,), k=10, rows=40, B=3, V=50, blank=0, ws=one,
             nbytes=1 << 20, n_hyp=one):
        hs = (ctypes.c_void_p * max(len(graphs), 1))(*[None if h is None else h.handle for h in graphs])
        return f(one, one, k, rows, one, one, B, V, blank, ints(*fb), ints(*sb), ints(*nb), ints(*go), hs, len(graphs), 8, n_hyp, one, one,
                 one, one, one, ws, nbytes, None)

    for bad in (dict(fb=(11, 0, 10)), dict(fb=(-1, 0, 10)), dict(fb=(3, 0, 17), k=16), dict(sb=(17, 0, 10)), dict(sb=(-1, 0, 10)),
                dict(nb=(0, 0, 4)), dict(nb=(6, 0, 4)), dict(sb=(0, 0, 10)), dict(go=(1, -1, -1)), dict(go=(0, -2, -1)),
                dict(go=(0, -1, 0), graphs=(g50, g49)), dict(graphs=(None,)), dict(k=0), dict(k=17), dict(blank=50), dict(blank=-1),
                dict(V=0), dict(rows=-1), dict(B=-1), dict(ws=None), dict(nbytes=8), dict(nbytes=48 + 48 + 64), dict(n_hyp=None)):
        assert call(**bad) == INVALID, bad


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_headers_compile(tmp_path, lang):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if cc is None:
        pytest.fail("no compiler to check the headers with")
    src = tmp_path / ("h.c" if lang == "c" else "h.cpp")
    src.write_text('#include "pfhip.h"\n#include "pfhip_ops.h"\n'
                   "int main(void) { pfhip_svs_beam_opts s; s.graph = 0; (void)s;\n"
                   "  return pfhip_op_ctc_prefix_beam_multi_workspace_bytes(0, 0, 1, 0, 0, 0, 0, 0, 0) != 0\n"
                   "      || pfhip_svs_forward_beam_sets(0, 0, 0, 0, 0, 0, 0, &s, 1, 0, 0) == PFHIP_OK; }\n")
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
