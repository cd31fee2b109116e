"""Dev tool (GPU): SHA-256 digests of everything the forwards return, one line per case, on synthetic weights and fixed seeds.
The kernels are deterministic, so two builds of the library whose host code enqueues the same launches print the same listing:
    python3 tools/forward_digest.py > new.txt;  PFHIP_LIB=build/ab/libpfhip_old.so python3 tools/forward_digest.py > old.txt;  diff old.txt new.txt
Every case is one short forward in a fresh child process (the path knobs are read once per process, from its environment).
Digested: token ids, token / fire / frame counts, log-probs, the `enc` and `alphas` tensors, and where the case has them the
timestamp head's us_alphas / us_cif_peak, the N-best ids and values, the streaming tokens with their per-token detail; for SenseVoice
everything pfhip_svs_forward returns from either CTC head, the rows' log-sum-exp and pfhip_svs_align on the returned tokens.  The debug
read-outs that tell which path ran (plane / exact / context counters) are printed beside the digest and must match as well.
    python3 tools/forward_digest.py [case ...]      (no argument: all cases)"""
import hashlib
import importlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PLANES = dict(PFHIP_PLANES_MIN_ROWS="1024", PFHIP_DEC_PLANES_MIN_ROWS="1")
# case -> the environment its child process adds
CASES = {
    "plain": {},
    "folded": {},
    "planes": PLANES,
    "planes_kv": dict(PLANES, PFHIP_KV_PLANES="1"),
    "planes_decoder": PLANES,         # enough token rows for the decoder's LayerNorm fold, which its plane path needs
    "side_stream": dict(PFHIP_DEC_SIDE="1"),
    "exact": {},
    "contextual_timestamp": {},
    "small_paraformer": {},
    "second_context": {},
    "streaming": {},
    "sensevoice": {},
    "sensevoice_logp": {},
}


class Digest:
    def __init__(self):
        self.h = hashlib.sha256()

    def add(self, *arrays):
        for a in arrays:
            a = np.ascontiguousarray(a)
            self.h.update(f"{a.dtype}{a.shape}".encode())
            self.h.update(a.tobytes())

    def add_forward(self, model, got, d_model):
        """one forward_ids result + the encoder-side tensors it left in the workspace"""
        self.add(got["token_num"], got["n_fires"], got["n_frames"])
        for key in ("ids", "logp", "us_alphas", "us_peaks"):
            for a in got.get(key) or []:
                self.add(a)
        for key in ("nbest_ids", "nbest_logp"):
            if key in got:
                self.add(got[key])
        rows = int(np.sum(got["n_frames"]))
        self.add(model.get_tensor("enc", rows * d_model), model.get_tensor("alphas", rows))


def run_case(name):
    import __graft_entry__ as ge
    from conftest import synth_pcm
    pkg = ge.load_package()
    W = importlib.import_module("asr_2pass_amd.weights")
    rng = np.random.default_rng(20251114)
    dg, notes = Digest(), {}
    secs = lambda *s: [synth_pcm(i, int(16000 * x) + 37 * i, rng) for i, x in enumerate(s)]
    if name in ("folded", "planes", "planes_kv", "planes_decoder", "side_stream", "exact"):
        man, blob = W.synth_weights(dict(W.PARAFORMER_LARGE), seed=1234)
        model = pkg.ParaformerHip().InitAsr((man, blob))
        utts = secs(*([16] * 16)) if name == "side_stream" else secs(*([30] * 12)) if name == "planes_decoder" else secs(24, 24, 24, 24)
        if name == "exact":
            model.debug_poke("range_flag", 1)           # the forward finds its range flag raised and is redone on the exact kernels
        dg.add_forward(model, model.forward_ids(utts, want_logp=True), 512)
        for key in ("plane_forwards", "dec_plane_forwards", "kvplane_forwards", "range_fallbacks"):
            notes[key] = model.debug_poke(key)
    elif name in ("plain", "second_context"):
        man, blob = W.synth_weights(W.small_config(), seed=1234)
        model = pkg.ParaformerHip().InitAsr((man, blob))
        utts = secs(1, 2.5, 4)
        if name == "second_context":
            model.set_inflight(2)
            for _ in range(2):                          # slots are taken in turn: the second call runs on context 1
                dg.add_forward(model, model.forward_ids(utts, want_logp=True), 512)
            notes["forwards_per_context"] = [s["forwards"] for s in model.inflight_stats()]
        else:
            dg.add_forward(model, model.forward_ids(utts, want_logp=True), 512)
            dg.add_forward(model, model.forward_ids(utts, want_logp=True, nbest=3), 512)
            for f in model.extract_feats(utts):
                dg.add(f)
    elif name == "contextual_timestamp":
        man, blob = W.synth_weights(W.small_config(enc_layers=2, dec_layers=2, vocab=400, contextual=1, timestamp=1), seed=1234)
        model = pkg.ParaformerHip().InitAsr((man, blob))
        sets = [model.CompileHotwordEmbedding([list(rng.integers(2, 400, n)) for n in lens]) for lens in ((2, 3, 4), (5, 2, 6, 3, 1))]
        dg.add(*sets)
        dg.add_forward(model, model.forward_ids(secs(3, 4), want_logp=True, want_timestamps=True, hw_sets=sets, set_of_utt=[0, 1]), 512)
    elif name == "small_paraformer":
        man, blob = W.synth_weights(W.small_config_320(), seed=1234)
        model = pkg.ParaformerHip().InitAsr((man, blob))
        dg.add_forward(model, model.forward_ids(secs(2, 3.5, 5), want_logp=True), 320)
    elif name == "streaming":
        man, blob = W.synth_weights(W.small_config(), seed=1234)
        model = pkg.ParaformerHip().InitAsr((man, blob))
        waves = secs(5, 5, 5, 5)

        def chunks(n):
            return [(k, min(k + 9600, n)) for k in range(0, n, 9600)]

        def add_detail(s, ids):
            det = s.last_detail()
            dg.add(np.asarray(ids, np.int32), det["ids"], det["logp"], det["fire_frame"])
        one = pkg.ParaformerOnlineHip(model)
        one.set_detail(3, True)
        for a, b in chunks(len(waves[0])):              # the latency path: one connection, one window per call
            add_detail(one, one.Forward(waves[0][a:b], input_finished=b == len(waves[0])))
        one.close()
        three = [pkg.ParaformerOnlineHip(model) for _ in range(3)]
        for s in three:
            s.set_detail(3, True)
        n = min(len(w) for w in waves[1:])
        for a, b in chunks(n):
            out = pkg.ParaformerOnlineHip.forward_batch(three, [w[a:b] for w in waves[1:]], [b == n] * 3)
            for s, ids in zip(three, out):
                add_detail(s, ids)
        for s in three:
            s.close()
    elif name in ("sensevoice", "sensevoice_logp"):
        model = pkg.SenseVoiceHip().InitAsr(W.synth_svs_weights(W.small_config_svs()))
        # without log-prob rows the fused CTC head runs, with them the unfused one (GEMM + log-softmax over row chunks)
        got = model.forward(secs(1, 2.5, 4), lid=[0, 3, 4], textnorm=[14, 15, 14], want_logp=name == "sensevoice_logp")
        dg.add(got["token_num"], got["frame_len"])
        for key in ("ids", "tok_frame", "tok_logp", "frame_ids", "frame_logp", "logp"):
            for a in got.get(key) or []:
                dg.add(a)
        rows = int(np.sum(got["frame_len"]))
        dg.add(model.get_tensor("enc", rows * 512), model.get_tensor("lse", rows))
        al = model.align([ids[4:] for ids in got["ids"]])              # the returned tokens after the four leading tags
        for key in ("begin", "end", "logp"):
            for a in al[key]:
                dg.add(a)
        dg.add(al["score"])
        for key in ("ctc_unfused_forwards", "ctc_head_chunks", "range_fallbacks", "plane_forwards"):
            notes[key] = model.debug_poke(key)
    else:
        raise SystemExit(f"unknown case {name}")
    model.close()
    print(f"{name:22s} {dg.h.hexdigest()}  {notes if notes else ''}".rstrip(), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--case":
        run_case(sys.argv[2])
        sys.exit(0)
    print("# library:", os.environ.get("PFHIP_LIB") or "in-tree", flush=True)
    for case in sys.argv[1:] or list(CASES):
        # a case that fails ends the listing: nothing more is started on a GPU that may just have faulted
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case], env=dict(os.environ, **CASES[case]), timeout=600).returncode
        if rc:
            sys.exit(f"case {case} ended with status {rc}")
