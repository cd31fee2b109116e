"""CPU: the entry points of the SenseVoice forward-with-spans and of the plan kernel are exported and bound, null arguments are
refused before any HIP call, and pfhip_svs_out — which callers allocate — keeps its layout."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["pfhip_svs_forward_spans", "pfhip_svs_forward_spans_s16", "pfhip_svs_set_batching"]
ERR_ARG = 1


@pytest.fixture(scope="module")
def lib(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg.load_lib()


def test_new_symbols_are_exported_and_bound(pkg, lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg.ABI_SYMBOLS, name
    assert hasattr(lib, "pfhip_op_ctc_greedy_plan")
    # pfhip_svs_forward's arguments plus the span buffer; the s16 form takes the same list
    assert lib.pfhip_svs_forward_spans.argtypes[:-1] == lib.pfhip_svs_forward.argtypes
    assert lib.pfhip_svs_forward_spans.argtypes[-1] == ctypes.POINTER(pkg._SvsAlignOut)
    assert lib.pfhip_svs_forward_spans_s16.argtypes == lib.pfhip_svs_forward_spans.argtypes


def test_null_arguments_are_refused_without_a_device(pkg, lib):
    out, sp = pkg._SvsOut(), pkg._SvsAlignOut()
    for fn in (lib.pfhip_svs_forward_spans, lib.pfhip_svs_forward_spans_s16):
        assert fn(None, None, None, 1, None, None, ctypes.byref(out), ctypes.byref(sp)) == ERR_ARG
        assert lib.pfhip_last_error() not in (None, b"")
    assert lib.pfhip_svs_set_batching(None, 100, 8) == ERR_ARG
    # the plan kernel's launcher checks its arguments before it launches anything (hipErrorInvalidValue = 1)
    assert lib.pfhip_op_ctc_greedy_plan(None, None, 4, 8, ctypes.c_longlong(100), None, None, None, None, None) == 1
    assert lib.pfhip_op_ctc_greedy_plan(None, None, -1, 8, ctypes.c_longlong(100), None, None, None, None, None) == 1


def test_pfhip_svs_out_keeps_its_layout(pkg, tmp_path):
    """Ten fields, 80 bytes on LP64, as before the span entry points: the spans have a struct of their own."""
    assert ctypes.sizeof(pkg._SvsOut) == 80 and pkg._SvsOut.logp_cap_floats.offset == 72
    assert ctypes.sizeof(pkg._SvsAlignOut) == 40
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler to check include/pfhip.h with")
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include "pfhip.h"\n'
                   "static_assert(sizeof(pfhip_svs_out) == 80, \"pfhip_svs_out changed size\");\n"
                   "static_assert(offsetof(pfhip_svs_out, max_tokens) == 16 && offsetof(pfhip_svs_out, frame_len) == 56 && "
                   "offsetof(pfhip_svs_out, logp_cap_floats) == 72, \"pfhip_svs_out changed layout\");\n"
                   "static_assert(sizeof(pfhip_svs_align_out) == 40, \"pfhip_svs_align_out changed size\");\n"
                   "static_assert(PFHIP_SVS_SPAN_MAX_FLOATS >= 96u * 500u * 501u, \"96 x 30 s must fit the span capacity\");\n"
                   "int main() { return 0; }\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
