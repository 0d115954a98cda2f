"""Time of the fused wav -> log-mel launch (csrc/audio_kernels.hip) on a speaker-sized bank: the first fixture recording repeated to about
20 k frames, HIP events around the launch; beside it the float32 torch.stft path on this box's CPU (context, not a gate).

    python tools/audio_bench.py [--copies 90] [--iters 20]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "maskcyclegan-vc_amd"), os.path.join(ROOT, "tests")]

from data_preprocessing.audio2mel import Audio2Mel, mel_filterbank, read_wav  # noqa: E402


def cpu_log_mel(x, basis, window):
    xp = torch.nn.functional.pad(x[None, None], (384, 384), "reflect")[0, 0]
    spec = torch.stft(xp, n_fft=1024, hop_length=256, win_length=1024, window=window, center=False, return_complex=True)
    return torch.log10(torch.clamp(basis @ spec.abs(), min=1e-5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=90)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    x = read_wav(os.path.join(ROOT, "tests", "golden", "audio", "real_VCC2SF3.wav"))
    fft = Audio2Mel()
    lengths = [x.size] * a.copies
    wave = torch.from_numpy(np.tile(x, a.copies)).cuda()
    out, fo = fft._launch(wave, lengths)                      # first call: basis upload, kernel attribute
    torch.cuda.synchronize()
    frames = int(fo[-1])
    ms = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out, _ = fft._launch(wave, lengths)                   # (plan + 16-byte-per-tile table upload + the launch)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    flop = frames * (2.0 * 1024 * 1024 + 4.0 * 513)
    print("bank: %d utterances, %d samples, %d frames, %.1f GFLOP" % (a.copies, wave.numel(), frames, flop / 1e9))
    print("GPU launch: median %.3f ms  min %.3f  max %.3f  -> %.1f TFLOP/s fp32 MFMA, %.1f M frames/s"
          % (ms[len(ms) // 2], ms[0], ms[-1], flop / ms[len(ms) // 2] / 1e9, frames / ms[len(ms) // 2] / 1e3))
    basis, window = torch.from_numpy(mel_filterbank()), torch.hann_window(1024)
    xt = torch.from_numpy(x)
    cpu_log_mel(xt, basis, window)
    t0 = time.perf_counter()
    for _ in range(a.copies):
        ref = cpu_log_mel(xt, basis, window)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    print("CPU float32 torch.stft path, same bank, %d threads: %.1f ms (%.0fx the launch)" % (torch.get_num_threads(), cpu_ms, cpu_ms / ms[len(ms) // 2]))
    print("max |GPU - CPU float32| on one utterance: %.2e" % float((out[:, :ref.shape[1]].cpu() - ref).abs().max()))


if __name__ == "__main__":
    main()
