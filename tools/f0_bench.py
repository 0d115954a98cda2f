"""Time of the HIP pitch tracker (csrc/f0_kernels.hip, mask_cyclegan_vc.pitch.PitchTracker) on a VCC2018-like evaluation set: a bank of 35
utterances of 150 .. 900 frames (the lengths of tools/dtw_bench.py's x side), lags 45 .. 367; HIP events around whole calls after a
warm-up (table upload and output allocation included: what a caller pays), beside the kernel alone through the C ABI on buffers made once,
with and without the d' output, and the CPU time of the float64 checker (tests/f0_checker.py) for ONE utterance.  Informational, not a
gate: there is nothing older to compare against.

    python tools/f0_bench.py [--iters 20] [--warmup 5] [--utts 35] [--fmin 60] [--fmax 500]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "maskcyclegan-vc_amd"), os.path.join(ROOT, "tests")]

import f0_checker as ck  # noqa: E402
from mask_cyclegan_vc import _hip, pitch  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--utts", type=int, default=35)
    ap.add_argument("--fmin", type=float, default=60.0)
    ap.add_argument("--fmax", type=float, default=500.0)
    a = ap.parse_args()
    rs = np.random.RandomState(0)
    frames = rs.randint(150, 901, size=a.utts)
    lengths = [int(256 * t) for t in frames]
    waves = []
    for n in lengths:                                                  # a vibrato tone plus noise per utterance: the time does not depend on the data
        t = np.arange(n) / ck.SR
        ph = 2 * np.pi * np.cumsum(rs.uniform(90, 300) * (1 + 0.03 * np.sin(2 * np.pi * 5 * t))) / ck.SR
        waves.append((0.2 * sum(np.sin(h * ph) / h for h in range(1, 6)) + 0.005 * rs.randn(n)).astype(np.float32))
    tr = pitch.PitchTracker(fmin=a.fmin, fmax=a.fmax)
    lo, hi = tr.lags
    total = int(frames.sum())
    wave = torch.from_numpy(np.concatenate(waves)).cuda()
    terms = total * 11.0 / 8.0 * 256 * (hi + 1)                        # (x[g] - x[g + tau])^2 terms the kernel evaluates: 11 hop blocks per 8 frames
    naive = float(total) * ck.W * (hi + 1)
    print("%d utterances, %d .. %d frames, %d frames in all, lags %d .. %d: %.3f G difference terms (frame by frame it would be %.3f G)"
          % (a.utts, frames.min(), frames.max(), total, lo, hi, terms / 1e9, naive / 1e9))
    med, lo_ms, hi_ms = timed(lambda: tr.track(wave, lengths), a.warmup, a.iters)
    print("PitchTracker.track: median %.3f ms (min %.3f max %.3f)" % (med, lo_ms, hi_ms))
    L = _hip.lib()
    offs = np.zeros(a.utts + 1, dtype=np.int32)
    np.cumsum(lengths, out=offs[1:])
    fo = np.zeros(a.utts + 1, dtype=np.int32)
    nt = ctypes.c_int(0)
    _hip.check(L.mcvc_audio_plan(offs.ctypes.data, a.utts, fo.ctypes.data, None, 0, ctypes.byref(nt)), "mcvc_audio_plan")
    tiles = np.zeros((nt.value, 4), dtype=np.int32)
    _hip.check(L.mcvc_audio_plan(offs.ctypes.data, a.utts, fo.ctypes.data, tiles.ctypes.data, nt.value, ctypes.byref(nt)), "mcvc_audio_plan")
    td = torch.from_numpy(tiles).cuda()
    f0 = torch.empty(total, dtype=torch.float32, device="cuda")
    apd = torch.empty(total, dtype=torch.float32, device="cuda")
    cm = torch.empty(hi + 1, total, dtype=torch.float32, device="cuda")
    for want_cmnd in (False, True):
        def raw():
            _hip.check(L.mcvc_f0_track(_hip.ptr(wave), int(offs[-1]), _hip.ptr(td), nt.value, lo, hi, tr.threshold, _hip.ptr(f0), _hip.ptr(apd),
                                       _hip.ptr(cm) if want_cmnd else None, total, _hip.stream()), "mcvc_f0_track")
        kmed, klo, khi = timed(raw, a.warmup, a.iters)
        print("kernel alone, d' output %-5s: median %.3f ms (min %.3f max %.3f) = %.2f T difference terms/s = %.1f TFLOP/s at 3 FLOP per term "
              "(subtract, multiply, add), %d workgroups" % (want_cmnd, kmed, klo, khi, terms / kmed / 1e9, 3.0 * terms / kmed / 1e9, nt.value * 8))
    voiced = int((f0 > 0).sum())
    t0 = time.perf_counter()
    f64 = ck.track(waves[0], lo, hi, tr.threshold)[0]
    dt = time.perf_counter() - t0
    got = f0[:int(frames[0])].cpu().numpy()
    both = (got > 0) & (f64 > 0)
    print("float64 checker on the CPU, ONE utterance of %d frames: %.2f s (the whole set at that rate: %.0f s); %d of %d frames voiced on the GPU; "
          "utterance 0: %d frames voiced in both, largest relative f0 difference %.2e"
          % (frames[0], dt, dt / frames[0] * total, voiced, total, int(both.sum()), float(np.abs(got[both] / f64[both] - 1).max()) if both.any() else 0.0))


if __name__ == "__main__":
    main()
