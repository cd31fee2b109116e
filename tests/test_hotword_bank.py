"""CPU: the bookkeeping of the hotword bank (csrc/hotword_bank.h: content hash + byte compare, LRU, pin counts, slab allocator) —
header-only host code, compiled here with g++ under AddressSanitizer / UBSan into csrc/host/hotword_bank_selftest.cpp's cases."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "asr-2pass_amd", "csrc", "host", "hotword_bank_selftest.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the hotword bank self-test")
    out = str(tmp_path_factory.mktemp("hwbank") / "hotword_bank_selftest")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                         SRC, "-o", out], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-4000:]
    return out


@pytest.mark.parametrize("case", ["collision",       # two sets with one hash: told apart by the byte compare
                                  "lru",             # the least recently used unpinned set goes first
                                  "pinned",          # a pinned slab survives pressure; allocation fails over to the per-call path
                                  "freelist",        # freed runs coalesce and are handed out again, entry ids too
                                  "unpin"])          # release on completion makes the slab evictable; reconfigure
def test_hotword_bank_bookkeeping(exe, case):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, case], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0 and out.stdout.strip() == f"ok {case}", out.stdout + out.stderr
