"""Writes the DNSMOS fixtures under tests/golden/:

  dnsmos_p808.npz, dnsmos_primary_<k>.npz   the REAL initialisers of utils/DNSMOS/model_v8.onnx and utils/DNSMOS/sig_bak_ovr.onnx under
                                            their ONNX names (data only: no graph is stored), the primary net's split in graph order so
                                            that no file exceeds 300 KB.  Needs the reference tree:
                                                python tests/golden/make_dnsmos_golden.py --weights /path/to/reference/utils
  dnsmos_cases.npz                          expected outputs of the three windows of tests/dnsmos_ref.py CASES (inputs are regenerated
                                            from seeds, not stored), from the fixtures above by the CPU restatement: `primary_f64`,
                                            `primary_f32` [3, 3], `p808_f64`, `p808_f32` [3, 1], and the mel input's checksum.
                                                python tests/golden/make_dnsmos_golden.py --cases
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CAP = 300 * 1024


def write_weights(utils_dir):
    import __graft_entry__ as ge
    ge.load_package()
    from asr_2pass_amd import onnx_reader
    for kind, rel in (("p808", "DNSMOS/model_v8.onnx"), ("primary", "DNSMOS/sig_bak_ovr.onnx")):
        m = onnx_reader.read_model(os.path.join(utils_dir, rel))
        # graph order: an initialiser is stored where the first node that reads it stands
        order = []
        for nd in m.nodes:
            for n in nd.inputs:
                if n in m.initializers and n not in order:
                    order.append(n)
        assert sorted(order) == sorted(m.initializers), "an initialiser no node reads"
        groups, cur, size = [], {}, 0
        for n in order:
            a = np.asarray(m.initializers[n])
            if cur and size + a.nbytes > CAP - 4096:
                groups.append(cur)
                cur, size = {}, 0
            cur[n] = a
            size += a.nbytes + 256
        groups.append(cur)
        if kind == "p808":
            assert len(groups) == 1
            np.savez(os.path.join(HERE, "dnsmos_p808.npz"), **groups[0])
        else:
            for i, g in enumerate(groups):
                np.savez(os.path.join(HERE, f"dnsmos_primary_{i}.npz"), **g)
        print(kind, [sum(a.nbytes for a in g.values()) for g in groups])


def write_cases():
    import dnsmos_ref as R
    Wp, W8 = R.load_weights("primary"), R.load_weights("p808")
    x = np.stack([R.case_window(c) for c in R.CASES])
    mel = np.stack([R.melspec(w[:R.MEL_SAMPLES]) for w in x])
    torch.set_num_threads(min(16, torch.get_num_threads()))
    out = dict(names=np.array(R.CASES))
    with torch.no_grad():
        out["primary_f64"] = R.primary_forward(Wp, x, torch.float64).numpy()
        out["primary_f32"] = R.primary_forward(Wp, x, torch.float32).numpy()
        out["p808_f64"] = R.p808_forward(W8, mel, torch.float64).numpy()
        out["p808_f32"] = R.p808_forward(W8, mel.astype(np.float32), torch.float32).numpy()
    out["mel_mean"] = mel.mean(axis=(1, 2))
    np.savez(os.path.join(HERE, "dnsmos_cases.npz"), **out)
    for k, v in out.items():
        print(k, v)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", metavar="UTILS_DIR", help="the reference tree's utils/ directory")
    ap.add_argument("--cases", action="store_true")
    a = ap.parse_args()
    if a.weights:
        write_weights(a.weights)
    if a.cases:
        write_cases()
