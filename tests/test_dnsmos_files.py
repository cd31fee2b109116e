"""CPU: DNSMOS .onnx files through the C++ reader inside libpfhip.so (csrc/mos_files.cpp, pfhip_read_model_files kind "dnsmos") and
through its Python twin (convert.convert_dnsmos): the two containers match bit for bit and hold the fixture tensors, for files written
from the fixtures by tests/dnsmos_onnx.py and, where the reference tree is present, for the real files (the personalised net
included).  The written files also run through the float64 graph walk and give the restatement's numbers, so the writer writes the
real topology.  Refusals: a truncated file, a file whose Conv kernel is missing, a graph of another family (a Paraformer block) and
a graph with the two STFT kernels under other names each give a status plus a message from BOTH readers, and the same files plus 300
damaged copies go through the reader built stand-alone with -fsanitize=address,undefined (tools/fuzz/dnsmos_files_check.cpp)."""
import os
import shutil
import subprocess
import wave

import numpy as np
import pytest

import dnsmos_onnx as O
import dnsmos_ref as R

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/utils"


@pytest.fixture(scope="module")
def mods(pkg):
    import importlib
    return pkg, importlib.import_module("asr_2pass_amd.convert"), importlib.import_module("asr_2pass_amd.dnsmos")


@pytest.fixture(scope="module")
def weights():
    return {k: R.load_weights(k) for k in ("primary", "p808")}


@pytest.fixture(scope="module")
def files(tmp_path_factory, weights):
    d = tmp_path_factory.mktemp("dnsmos_files")
    good = O.primary_onnx(weights["primary"])
    blobs = {
        "primary": good,
        "p808": O.p808_onnx(weights["p808"]),
        "truncated": good[:len(good) // 2],
        "kernel_missing": O.primary_onnx(weights["primary"], drop=("conv2d_3/kernel:0",)),
        "other_family": O.not_dnsmos_onnx(),
        "stft_renamed": O.primary_onnx({k.replace("stft-real", "stft-a").replace("stft-imag", "stft-b"): v for k, v in weights["primary"].items()},
                                       rename={"time2freq/stft-real/kernel:0": "time2freq/stft-a/kernel:0",
                                               "time2freq/stft-imag/kernel:0": "time2freq/stft-b/kernel:0"}),
    }
    out = {}
    for k, b in blobs.items():
        out[k] = str(d / f"{k}.onnx")
        with open(out[k], "wb") as f:
            f.write(b)
    return out


def tensor(man, blob, name):
    t = man["tensors"][name]
    n = int(np.prod(t["shape"]))
    return blob[t["offset"] // 4:t["offset"] // 4 + n].reshape(t["shape"])


def check_container(man, blob, Wp, W8):
    assert man["config"]["kind"] == "dnsmos" and man["config"]["has_p808"] == (1 if W8 is not None else 0)
    assert man["config"]["primary_convs"] == [v for n, p in R.PRIMARY["convs"] for v in (*Wp[f"{n}/kernel:0"].shape[:2], int(p))]
    assert tensor(man, blob, "primary.stft_real").tobytes() == Wp["time2freq/stft-real/kernel:0"].tobytes()
    assert tensor(man, blob, "primary.stft_imag").tobytes() == Wp["time2freq/stft-imag/kernel:0"].tobytes()
    assert list(tensor(man, blob, "primary.consts")) == [np.float32(1e-12), np.float32(2.0), np.float32(2.3025851)]
    for pre, W, net in (("primary", Wp, R.PRIMARY), ("p808", W8, R.P808)):
        if W is None:
            continue
        for i, (n, _) in enumerate(net["convs"]):
            assert tensor(man, blob, f"{pre}.conv{i}.w").tobytes() == W[f"{n}/kernel:0"].tobytes()
            assert tensor(man, blob, f"{pre}.conv{i}.b").tobytes() == W[f"{n}/bias:0"].tobytes()
        for i, d in enumerate(net["dense"]):
            p = f"{net['prefix']}/{d}"
            assert tensor(man, blob, f"{pre}.dense{i}.w").tobytes() == W[f"{p}/MatMul/ReadVariableOp/resource:0"].tobytes()
            assert tensor(man, blob, f"{pre}.dense{i}.b").tobytes() == W[f"{p}/BiasAdd/ReadVariableOp/resource:0"].tobytes()


def both_readers(mods, primary, p808=None):
    pkg, conv, _ = mods
    man, blob, _ = pkg.read_model_files("dnsmos", primary, second=p808)
    man2, blob2 = conv.convert_dnsmos(primary, p808)
    assert man["config"] == man2["config"] and man["tensors"] == man2["tensors"] and man["total_bytes"] == man2["total_bytes"]
    assert blob.tobytes() == blob2.tobytes()
    return man, blob


def test_written_files_cpp_reader_equals_converter(mods, files, weights):
    man, blob = both_readers(mods, files["primary"], files["p808"])
    check_container(man, blob, weights["primary"], weights["p808"])
    man, blob = both_readers(mods, files["primary"])
    check_container(man, blob, weights["primary"], None)


def test_written_graphs_compute_what_the_restatement_computes(mods, files, weights):
    from asr_2pass_amd import onnx_reader
    x = R.case_window("tone_noise")[None]
    with torch.no_grad():
        env = R.walk_graph(onnx_reader.read_model(files["primary"]), {"input_1": x})
        assert np.abs(env["Identity:0"].numpy() - R.primary_forward(weights["primary"], x).numpy()).max() < 1e-12
        mel = R.melspec(x[0, :R.MEL_SAMPLES])[None]
        env = R.walk_graph(onnx_reader.read_model(files["p808"]), {"input_1": mel})
        assert np.abs(env["Identity:0"].numpy() - R.p808_forward(weights["p808"], mel).numpy()).max() < 1e-12


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "DNSMOS/sig_bak_ovr.onnx")), reason="/root/reference not present")
def test_real_files_cpp_reader_equals_converter(mods, weights):
    P, Q = os.path.join(REF, "DNSMOS/sig_bak_ovr.onnx"), os.path.join(REF, "DNSMOS/model_v8.onnx")
    man, blob = both_readers(mods, P, Q)
    check_container(man, blob, weights["primary"], weights["p808"])
    # the personalised net: the same skeleton with its own weights
    man2, blob2 = both_readers(mods, os.path.join(REF, "pDNSMOS/sig_bak_ovr.onnx"))
    assert man2["config"]["primary_convs"] == man["config"]["primary_convs"]
    assert tensor(man2, blob2, "primary.conv1.w").tobytes() != tensor(man, blob, "primary.conv1.w").tobytes()


@pytest.mark.parametrize("name, word", [("truncated", ""), ("kernel_missing", "conv2d_3"), ("other_family", "LayerNormalization"),
                                        ("stft_renamed", "stft-a")])
def test_refusals_give_a_status_and_a_message(mods, files, name, word):
    pkg, conv, _ = mods
    with pytest.raises(pkg.PfhipError, match="pfhip status 3") as e:
        pkg.read_model_files("dnsmos", files[name])
    assert word in str(e.value) and len(str(e.value)) > len("pfhip status 3: ")
    with pytest.raises((pkg.PfhipError, ValueError)) as e2:
        conv.convert_dnsmos(files[name])
    assert word in str(e2.value)
    # the P.808 file as the primary net, and the primary as the P.808 net
    with pytest.raises(pkg.PfhipError, match="front end"):
        pkg.read_model_files("dnsmos", files["p808"])
    with pytest.raises(pkg.PfhipError, match="Slice"):
        pkg.read_model_files("dnsmos", files["primary"], second=files["primary"])


def test_damaged_files_under_address_sanitizer(files, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "dnsmos_files_check")
    csrc = os.path.join(ROOT, "asr-2pass_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tools", "fuzz", "dnsmos_files_check.cpp"), os.path.join(csrc, "model_files.cpp"),
                        os.path.join(csrc, "mos_files.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in ("truncated", "kernel_missing", "other_family", "stft_renamed"):
        r = subprocess.run([exe, "primary", files[name]], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("refused: ") and len(r.stdout) > 12, (name, r.stdout, r.stderr[-2000:])
    r = subprocess.run([exe, "primary", files["primary"], "200", "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("loaded ") and "damaged:" in r.stdout, (r.stdout, r.stderr[-2000:])
    r = subprocess.run([exe, "p808", files["p808"], files["primary"], "100", "8"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("loaded ") and "damaged:" in r.stdout, (r.stdout, r.stderr[-2000:])


def test_window_arithmetic_of_the_package(mods):
    """dnsmos.windows_of (what sizes the caller's buffer) against the issue's known answers; the C++ loop itself is held against these
    counts on the GPU (tests/test_gpu_dnsmos.py)."""
    _, _, dnsmos = mods
    assert dnsmos.windows_of(9 * 16000) == (18 * 16000, 9, 7)
    assert dnsmos.windows_of(600 * 16000) == (600 * 16000, 591, 570)
    assert dnsmos.windows_of(144160) == (144160, 1, 1)
    assert dnsmos.windows_of(175999) == (175999, 1, 1)
    assert dnsmos.windows_of(1)[:2] == (1 << 18, 7)
    for n in (1, 9 * 16000, 175999, 600 * 16000):
        ext, hops, kept = dnsmos.windows_of(n)
        assert (hops, kept) == (R.clip_windows(ext)[0], len(R.clip_windows(ext)[1]))
    with pytest.raises(mods[0].PfhipError):
        dnsmos.windows_of(0)


def test_score_tool_reads_riff(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("dnsmos_score", os.path.join(ROOT, "tools", "dnsmos_score.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    pcm = (np.arange(2000) % 300 - 150).astype("<i2")
    p = str(tmp_path / "a.wav")
    with wave.open(p, "wb") as wf:
        wf.setnchannels(2)
        wf.setsampwidth(2)
        wf.setframerate(8000)
        wf.writeframes(np.stack([pcm, -pcm], axis=1).tobytes())
    x, fs = tool.read_wav(p)
    assert fs == 8000 and x.dtype == np.int16 and np.array_equal(x, pcm)
    assert tool.format_line("utt1", 3.14159) == "utt1\t3.1416\n"
