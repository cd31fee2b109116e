"""Dev tool (GPU): the frame-energy kernel (csrc/vad_energy.hip) against the host loop it replaces.
Kernel time by HIP events (median of 20 launches after 3 warm-ups) on one 600-s file and on 32 x 30 s, f32 and s16; the host
loop's wall time on the same audio is the difference between pfhip_vadseg_feed (waveform: 400 dependent adds per frame, then
the detector) and pfhip_vadseg_feed_energy (the detector alone) on one core.  PFHIP_ENERGY_PAD=0 times the unpadded LDS image."""
import ctypes, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge
pkg = ge.load_package()
import importlib, torch
ops = importlib.import_module("asr_2pass_amd.ops")
from conftest import synth_pcm

rng = np.random.default_rng(7)


def kernel_ms(pcm, lens):
    lib = ops._lib()
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    nf = np.array([0 if n < 400 else 1 + (n - 400) // 160 for n in lens], np.int32)
    fo = np.concatenate([[0], np.cumsum(nf)]).astype(np.int32)
    d, d_off, d_fo, d_nf = (torch.from_numpy(a).cuda() for a in (pcm, off, fo, nf))
    e = torch.empty(int(fo[-1]), dtype=torch.float32, device="cuda")
    ops.frame_energy(d[:1000], [0], [1000])                    # binds the argument types
    fn = lib.pfhip_op_frame_energy_s16 if pcm.dtype == np.int16 else lib.pfhip_op_frame_energy
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ts = []
    for it in range(23):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn(d.data_ptr(), d_off.data_ptr(), d_fo.data_ptr(), d_nf.data_ptr(), len(lens), int(fo[-1]), 400, 160, e.data_ptr(), st)
        b.record()
        torch.cuda.synchronize()
        assert rc == 0
        if it >= 3:
            ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), e.cpu().numpy()


def host_loop_ms(pcm_f32, energy):
    F = energy.size
    sil = np.full(F, 0.9, np.float32)
    n = 400 + 160 * (F - 1)
    best = [1e9, 1e9]
    for _ in range(3):
        m = pkg.E2EVadModelHost()
        t0 = time.perf_counter(); m(sil, pcm_f32[:n], True, False); t1 = time.perf_counter()
        m.feed_energy(sil, energy, n, True, False); t2 = time.perf_counter()
        m.close()
        best = [min(best[0], t1 - t0), min(best[1], t2 - t1)]
    return 1e3 * best[0], 1e3 * best[1]


for name, lens in (("1 x 600 s", [600 * 16000]), ("32 x 30 s", [30 * 16000] * 32)):
    f32 = np.concatenate([synth_pcm(i, n, rng) for i, n in enumerate(lens)])
    s16 = np.round(f32 * 32768.0).astype(np.int16)
    for fmt, x in (("f32", f32), ("s16", s16)):
        med, mn, e = kernel_ms(x, lens)
        print(f"{name} {fmt}: kernel median {1e3 * med:.1f} us (min {1e3 * mn:.1f} us), {e.size} frames, pad={os.environ.get('PFHIP_ENERGY_PAD', '1')}", flush=True)
    if os.environ.get("PFHIP_ENERGY_PAD", "1") != "0":
        if len(lens) == 1:
            w, d = host_loop_ms(f32, e)
            print(f"{name}: host detector on the waveform {w:.2f} ms, on energies {d:.2f} ms -> decibel loop {w - d:.2f} ms on one core", flush=True)
        else:
            tw = td = 0.0
            for i, n in enumerate(lens):
                seg = f32[i * n:(i + 1) * n]
                w, d = host_loop_ms(seg, e[i * (e.size // len(lens)):(i + 1) * (e.size // len(lens))])
                tw += w; td += d
            print(f"{name}: host detector on the waveforms {tw:.2f} ms, on energies {td:.2f} ms -> decibel loops {tw - td:.2f} ms on one core", flush=True)
