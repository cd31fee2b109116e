"""Dev tool (GPU): what pfhip_stream_set_detail costs.  One connection fed 600-ms chunks (median ms per chunk) and a round of N
connections through pfhip_stream_forward_batch (median ms per round), with the Paraformer-large-sized online model (random-init):

  python tools/stream_detail_bench.py [k=0] [fires=0] [chunks=150] [connections=128] [rounds=24]

k = 0 and fires = 0 never call the setter, so the run also works with an older library given through PFHIP_LIB (the baseline of
an A/B run: alternate the two inside one session).  Prints one line per leg."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
weights = importlib.import_module("asr_2pass_amd.weights")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import synth_pcm  # noqa: E402

k = int(sys.argv[1]) if len(sys.argv) > 1 else 0
fires = bool(int(sys.argv[2])) if len(sys.argv) > 2 else False
chunks = int(sys.argv[3]) if len(sys.argv) > 3 else 150
B = int(sys.argv[4]) if len(sys.argv) > 4 else 128
rounds = int(sys.argv[5]) if len(sys.argv) > 5 else 24
tag = f"lib={os.path.basename(os.environ.get('PFHIP_LIB', 'in-tree'))} k={k} fires={int(fires)}"

model = pkg.ParaformerHip().InitAsr(weights.synth_weights(dict(weights.PARAFORMER_LARGE), seed=1234))
rng = np.random.default_rng(20251114)


def new_stream():
    s = pkg.ParaformerOnlineHip(model)
    if k or fires:
        s.set_detail(k, fires)
    return s


def read_detail(s):
    return s.last_detail() if (k or fires) else None


pcm = synth_pcm(0, 9600 * chunks, rng)
s = new_stream()
for j in range(3):
    s.Forward(pcm[j * 9600:(j + 1) * 9600], input_finished=False)
s.Reset()
lat, ntok = [], 0
for j in range(chunks):
    t1 = time.perf_counter()
    ids = s.Forward(pcm[j * 9600:(j + 1) * 9600], input_finished=(j == chunks - 1))
    read_detail(s)
    lat.append(time.perf_counter() - t1)
    ntok += len(ids)
lat = np.asarray(lat) * 1e3
print(f"{tag} one connection: per-chunk ms median {np.median(lat):.3f} p10 {np.percentile(lat, 10):.3f} p90 {np.percentile(lat, 90):.3f} "
      f"({chunks} chunks, {ntok} tokens)", flush=True)
s.close()

streams = [new_stream() for _ in range(B)]
waves = [synth_pcm(i, 9600 * rounds, rng) for i in range(B)]
for j in range(2):
    pkg.ParaformerOnlineHip.forward_batch(streams, [w[j * 9600:(j + 1) * 9600] for w in waves], [False] * B)
lat, ntok = [], 0
for j in range(2, rounds):
    t1 = time.perf_counter()
    res = pkg.ParaformerOnlineHip.forward_batch(streams, [w[j * 9600:(j + 1) * 9600] for w in waves], [False] * B)
    for x in streams:
        read_detail(x)
    lat.append(time.perf_counter() - t1)
    ntok += sum(len(r) for r in res)
lat = np.asarray(lat) * 1e3
print(f"{tag} {B} connections: per-round ms median {np.median(lat):.3f} p10 {np.percentile(lat, 10):.3f} p90 {np.percentile(lat, 90):.3f} "
      f"({rounds - 2} rounds, {ntok} tokens, {ntok / (rounds - 2):.1f} per round)", flush=True)
for x in streams:
    x.close()
model.close()
