"""CPU: the bookkeeping of the bank of hotword context graphs (csrc/graph_bank.h over csrc/hotword_bank.h), keyed by the packed
images of graphs the real builder made (csrc/ctx_graph.cpp) — host code only, compiled here with plain g++ into
csrc/host/graph_bank_selftest.cpp's cases (`make graph_bank_selftest` builds and runs the same program under ASan / UBSan)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-2pass_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the graph bank self-test")
    out = str(tmp_path_factory.mktemp("graphbank") / "graph_bank_selftest")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(CSRC, "ctx_graph.cpp"),
                         os.path.join(CSRC, "host", "graph_bank_selftest.cpp"), "-o", out], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-4000:]
    return out


@pytest.mark.parametrize("case", ["hit_miss",        # a graph goes in once; another handle with the same content finds it
                                  "pinned",          # a pinned image survives pressure; the newcomer is refused until a release
                                  "lru",             # the least recently used unpinned image goes first
                                  "refusal",         # a bank of 0 bytes, an image larger than the bank
                                  "collision",       # two contents under one forced hash: told apart by the byte compare
                                  "padding"])        # the row count is part of the key
def test_graph_bank_bookkeeping(exe, case):
    out = subprocess.run([exe, case], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == f"ok {case}", out.stdout + out.stderr
