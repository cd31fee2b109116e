"""CPU: SenseVoiceSmallHip compiles against the reference's REAL base classes, as tests/test_ref_headers.py checks the other
adapters: `g++ -fsyntax-only -Werror=overloaded-virtual -DPFHIP_WITH_FUNASR` on sensevoice_hip.cpp with model.h /
wfst-decodable.h / decoder.h / vocab.h from /root/reference, plus a translation unit of static_asserts (derives from funasr::Model
and funasr::WfstDecodable, is not abstract, and the call offline-stream / funasrruntime.cpp:265-266 make through the base pointer —
the svs_lang / svs_itn overload of model.h:33-34 — reaches the adapter's override).  Skipped where /root/reference does not exist."""
import os
import subprocess

import pytest

from test_ref_headers import HOST, ORT, include_flags  # noqa: F401  (the fixture that generates gflags.h and lists the include dirs)

pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(ORT, "include")), reason="/root/reference not present")
FLAGS = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Werror=overloaded-virtual", "-DPFHIP_WITH_FUNASR"]


def test_adapter_compiles_against_reference_headers(include_flags):
    r = subprocess.run(FLAGS + include_flags + [os.path.join(HOST, "sensevoice_hip.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


def test_adapter_is_a_model_and_overrides_the_svs_forward(include_flags, tmp_path):
    src = tmp_path / "seam.cpp"
    src.write_text('#include "sensevoice_hip.h"\n'
                   "#include <type_traits>\n"
                   "using funasr::SenseVoiceSmallHip;\n"
                   'static_assert(std::is_base_of<funasr::Model, SenseVoiceSmallHip>::value, "not a Model");\n'
                   'static_assert(std::is_base_of<funasr::WfstDecodable, SenseVoiceSmallHip>::value, "not a WfstDecodable");\n'
                   'static_assert(!std::is_abstract<SenseVoiceSmallHip>::value, "abstract");\n'
                   "std::vector<std::string> through_the_base(funasr::Model* m, float** din, int* len) {\n"
                   '  return m->Forward(din, len, true, std::string("en"), true, nullptr, 2);      // funasrruntime.cpp:265-266\n'
                   "}\n"
                   "void init_through_the_base(funasr::Model* m, const std::string& s) { m->InitAsr(s, s, s, s, 1); }      // offline-stream.cpp:89\n")
    r = subprocess.run(FLAGS + include_flags + ["-I" + HOST, str(src)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


def test_the_check_really_sees_the_reference_base_class(include_flags, tmp_path):
    """Negative control: an adapter whose SenseVoice Forward drifted from model.h:33-34 (bool svs_itn -> int) must be rejected."""
    bad = tmp_path / "drift.cpp"
    bad.write_text('#include "model.h"\n'
                   "struct Drift : funasr::Model {\n"
                   "  void StartUtterance() override {} void EndUtterance() override {} void Reset() override {}\n"
                   "  std::string Rescoring() override { return \"\"; } int GetAsrSampleRate() override { return 16000; }\n"
                   "  std::vector<std::string> Forward(float** din, int* len, bool fin, std::string svs_lang, int svs_itn, void* dec,\n"
                   "                                   int batch_in) override { return {}; }\n"
                   "};\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only"] + include_flags + [str(bad)], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "override" in r.stderr
