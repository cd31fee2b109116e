"""CPU: the 2-pass seam of SenseVoiceSmallHip against the reference's REAL headers, as tests/test_sensevoice_headers.py checks its
offline seam: `g++ -fsyntax-only -DPFHIP_WITH_FUNASR` with model.h / wfst-decodable.h / decoder.h / vocab.h from /root/reference.
The calls are those TpassStream and TpassOnlineStream make: the nine-argument InitAsr through a `funasr::Model*`
(tpass-stream.cpp:76-77), InitLm (:92-98) and `ParaformerOnlineHip(model, chunk_size, MODEL_SVS)` (paraformer-online.cpp:12-62).
Skipped where /root/reference does not exist."""
import os
import subprocess

import pytest

from test_ref_headers import HOST, ORT, include_flags  # noqa: F401  (the fixture that generates gflags.h and lists the include dirs)

pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(ORT, "include")), reason="/root/reference not present")
FLAGS = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Werror=overloaded-virtual", "-DPFHIP_WITH_FUNASR"]


def test_both_adapters_compile_against_reference_headers(include_flags):
    for name in ("sensevoice_hip.cpp", "paraformer_hip.cpp"):
        r = subprocess.run(FLAGS + include_flags + [os.path.join(HOST, name)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, name + "\n" + r.stderr[-4000:]


def test_the_tpass_calls_reach_the_adapter(include_flags, tmp_path):
    src = tmp_path / "tpass_seam.cpp"
    src.write_text('#include "sensevoice_hip.h"\n'
                   "#include <type_traits>\n"
                   "using funasr::SenseVoiceSmallHip;\n"
                   "using S = const std::string&;\n"
                   "// the adapter OVERRIDES the nine- and eight-argument forms of model.h:23-26, it does not merely inherit the empty ones\n"
                   "using Nine = void (SenseVoiceSmallHip::*)(S, S, S, S, S, S, S, int, S);\n"
                   "using Eight = void (SenseVoiceSmallHip::*)(S, S, S, S, S, S, S, int);\n"
                   "static_assert(std::is_same<decltype(static_cast<Nine>(&SenseVoiceSmallHip::InitAsr)), Nine>::value, \"no nine-argument InitAsr\");\n"
                   "static_assert(std::is_same<decltype(static_cast<Eight>(&SenseVoiceSmallHip::InitAsr)), Eight>::value, \"no eight-argument InitAsr\");\n"
                   'static_assert(std::is_base_of<funasr::OnlineModelOwner, SenseVoiceSmallHip>::value, "holds no online model");\n'
                   'static_assert(std::is_base_of<funasr::OnlineModelOwner, funasr::ParaformerHip>::value, "holds no online model");\n'
                   "void tpass_stream(S s) {\n"
                   "  SenseVoiceSmallHip* svs = new SenseVoiceSmallHip();\n"
                   "  funasr::Model* asr_handle = svs;                                   // tpass-stream.cpp:44-50\n"
                   "  asr_handle->InitAsr(s, s, s, s, s, s, s, 1, s);                    // :76-77\n"
                   "  asr_handle->InitAsr(s, s, s, s, s, s, s, 1);\n"
                   "  asr_handle->InitLm(s, s, s, s);                                    // :92-98\n"
                   "  asr_handle->InitLm(s, s, s);\n"
                   '  funasr::ParaformerOnlineHip online(asr_handle, {5, 10, 5}, "SenseVoiceSmall");      // tpass-online-stream.cpp:14-15\n'
                   "  funasr::Model* m = &online;\n"
                   "  (void)m; (void)svs->OnlineHandle();\n"
                   "}\n")
    r = subprocess.run(FLAGS + include_flags + ["-I" + HOST, str(src)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


def test_a_wrong_signature_is_rejected(include_flags, tmp_path):
    """Negative control: a nine-argument InitAsr whose thread_num drifted to a string is no override of model.h:25-26."""
    bad = tmp_path / "drift.cpp"
    bad.write_text('#include "model.h"\n'
                   "using S = const std::string&;\n"
                   "struct Drift : funasr::Model {\n"
                   "  void StartUtterance() override {} void EndUtterance() override {} void Reset() override {}\n"
                   "  std::string Rescoring() override { return \"\"; } int GetAsrSampleRate() override { return 16000; }\n"
                   "  void InitAsr(S am, S en, S de, S cmvn, S cfg, S tok, S otok, S thread_num, S ocfg) override {}\n"
                   "};\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only"] + include_flags + [str(bad)], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "override" in r.stderr
