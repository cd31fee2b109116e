"""Clip-level DNSMOS scores on the GPU with the reference script's arguments (utils/dnsmos_local.py): a wav.scp in, `utt\\tmos` with four
decimals out (the mean P.808 MOS over the scored windows).

    python tools/dnsmos_score.py -i wav.scp -o mos.txt --model-dir /path/to/utils [-p] [--batch 16]

--model-dir holds DNSMOS/sig_bak_ovr.onnx, DNSMOS/model_v8.onnx and, for -p, pDNSMOS/sig_bak_ovr.onnx.  RIFF files are read with the
`wave` module (16-bit PCM, first channel); a file that is not 16 kHz goes through pfhip_resample first — Kaldi's resampler, where the
reference script calls librosa's, so its scores differ from the script's by that much."""
import argparse
import os
import sys
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_wav(path):
    with wave.open(path) as wf:
        if wf.getsampwidth() != 2:
            raise ValueError(f"{path}: 16-bit PCM expected")
        a = np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2").reshape(-1, wf.getnchannels())[:, 0]
        return np.ascontiguousarray(a), wf.getframerate()


def format_line(utt, mos):
    """The reference script's output line: `utt\tmos` with four decimals."""
    return f"{utt}\t{mos:.04f}\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--wav_scp", required=True)
    ap.add_argument("-o", "--mos_res", required=True)
    ap.add_argument("-p", "--personalized_MOS", action="store_true")
    ap.add_argument("--model-dir", required=True)
    ap.add_argument("--batch", type=int, default=16, help="clips per call")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    from asr_2pass_amd import ops
    primary = os.path.join(a.model_dir, "pDNSMOS" if a.personalized_MOS else "DNSMOS", "sig_bak_ovr.onnx")
    mos = pkg.DnsMosHip().InitMos(primary, os.path.join(a.model_dir, "DNSMOS", "model_v8.onnx"))
    clips = [line.strip().split(maxsplit=1) for line in open(a.wav_scp) if line.strip()]
    with open(a.mos_res, "w", encoding="utf-8") as out:
        for i in range(0, len(clips), a.batch):
            names, pcm = [], []
            for utt, path in clips[i:i + a.batch]:
                x, fs = read_wav(path)
                if fs != 16000:
                    y, _, _ = ops.resample(torch.as_tensor(x.astype(np.float32) / np.float32(32768.0)).cuda(), [0], [x.size], fs)
                    pcm.append(y.cpu().numpy())
                else:
                    pcm.append(x)
                names.append(utt)
            # one call takes one sample type: resampled clips are float32, so convert the rest where a batch mixes them
            if len({p.dtype for p in pcm}) > 1:
                pcm = [p if p.dtype == np.float32 else p.astype(np.float32) / np.float32(32768.0) for p in pcm]
            for utt, r in zip(names, mos.score(pcm, a.personalized_MOS)):
                out.write(format_line(utt, r["p808"]))
                out.flush()
    mos.close()


if __name__ == "__main__":
    main()
