"""CPU: pfhip_svs_forward_beam[_s16] are exported and bound, null arguments are refused before any HIP call, and the two structs
callers allocate have the layout the Python binding assumes."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["pfhip_svs_forward_beam", "pfhip_svs_forward_beam_s16"]
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
    assert lib.pfhip_svs_forward_beam.argtypes[:-2] == lib.pfhip_svs_forward.argtypes
    assert lib.pfhip_svs_forward_beam.argtypes[-2:] == [ctypes.POINTER(pkg._SvsBeamOpts), ctypes.POINTER(pkg._SvsBeamOut)]
    assert lib.pfhip_svs_forward_beam_s16.argtypes == lib.pfhip_svs_forward_beam.argtypes


def test_null_arguments_are_refused_without_a_device(pkg, lib):
    out, opts, bo = pkg._SvsOut(), pkg._SvsBeamOpts(3, 3, 3, None), pkg._SvsBeamOut()
    for fn in (lib.pfhip_svs_forward_beam, lib.pfhip_svs_forward_beam_s16):
        assert fn(None, None, None, 1, None, None, ctypes.byref(out), ctypes.byref(opts), ctypes.byref(bo)) == ERR_ARG
        assert lib.pfhip_last_error() not in (None, b"")


def test_struct_layouts(pkg, tmp_path):
    assert ctypes.sizeof(pkg._SvsBeamOpts) == 24 and pkg._SvsBeamOpts.graph.offset == 16
    assert ctypes.sizeof(pkg._SvsBeamOut) == 56 and pkg._SvsBeamOut.max_tokens.offset == 48
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler to check include/pfhip.h with")
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include "pfhip.h"\n'
                   "static_assert(sizeof(pfhip_svs_beam_opts) == 24 && offsetof(pfhip_svs_beam_opts, graph) == 16, \"pfhip_svs_beam_opts\");\n"
                   "static_assert(sizeof(pfhip_svs_beam_out) == 56 && offsetof(pfhip_svs_beam_out, n_tokens) == 16 && "
                   "offsetof(pfhip_svs_beam_out, max_tokens) == 48, \"pfhip_svs_beam_out\");\n"
                   "static_assert(sizeof(pfhip_svs_out) == 80, \"pfhip_svs_out changed size\");\n"
                   "int main() { return 0; }\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
