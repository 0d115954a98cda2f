"""Time of the modulation-spectrum kernels (csrc/ms_kernels.hip, mask_cyclegan_vc.metrics.modulation_spectrum / msd) on a VCC2018-like
evaluation set: 35 utterances of 150 .. 900 frames (the lengths of tools/dtw_bench.py's x side), K = 24, n_fft = 4096.  HIP events around
whole calls after a warm-up (bank building, offset upload and output allocation included: what a caller pays), beside the ms_power kernel
alone through the C ABI on buffers made once (many launches per timed window), beside ``torch.fft.rfft`` of the zero-padded, mean-removed
bank on the same device as a yardstick, and the CPU time of the float64 checker (tests/ms_checker.py) for the same set.  Informational,
not a gate: there is nothing older to compare against.

    python tools/ms_bench.py [--iters 20] [--warmup 5] [--utts 35] [--n_fft 4096] [--out profiles/ms_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "maskcyclegan-vc_amd"), os.path.join(ROOT, "tests")]

import ms_checker as ck  # noqa: E402
from mask_cyclegan_vc import _hip, metrics  # noqa: E402


def timed(fn, warmup, iters, inner=1):
    """-> (median, min, max) ms per call of ``fn``; ``inner`` calls between one pair of events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--utts", type=int, default=35)
    ap.add_argument("--n_cep", type=int, default=24)
    ap.add_argument("--n_fft", type=int, default=4096)
    ap.add_argument("--out", type=str, default=None, help="also write the figures to this JSON file")
    a = ap.parse_args()
    rs = np.random.RandomState(0)
    frames = rs.randint(150, 901, size=a.utts)
    mels = [(-2.0 + np.cumsum(0.05 * rs.randn(80, T), axis=1) + 0.1 * rs.randn(80, T)).astype(np.float32) for T in frames]
    mels_b = [(-2.0 + np.cumsum(0.05 * rs.randn(80, T), axis=1) + 0.2 * rs.randn(80, T)).astype(np.float32) for T in frames[::-1]]
    K, n_fft, nb, total = a.n_cep, a.n_fft, a.n_fft // 2, int(frames.sum())
    flop = 4.0 * K * total * nb                                         # two components, one multiply-add each, per row, frame and bin
    flop_tiles = 4.0 * 32 * ((K + 31) // 32) * float(sum(2 * ((min(64, T - t0) + 1) // 2) for T in frames for t0 in range(0, T, 64))) * nb
    res = {"device": torch.cuda.get_device_name(0), "utterances": a.utts, "frames_min": int(frames.min()), "frames_max": int(frames.max()),
           "frames_total": total, "K": K, "n_fft": n_fft, "iters": a.iters, "warmup": a.warmup, "gflop": flop / 1e9, "gflop_issued_in_mfma_tiles": flop_tiles / 1e9,
           "launches_msd": int(_hip.lib().mcvc_ms_launches())}
    print("%d utterances, %d .. %d frames, %d frames in all, K = %d, n_fft = %d: %.2f GFLOP (%.2f issued in 32-row MFMA tiles)"
          % (a.utts, frames.min(), frames.max(), total, K, n_fft, flop / 1e9, flop_tiles / 1e9))

    cep, offs = metrics.mel_cepstra(mels, K)
    med, lo, hi = timed(lambda: metrics.modulation_spectrum((cep, offs), n_fft), a.warmup, a.iters)
    res["modulation_spectrum_ms"] = {"median": med, "min": lo, "max": hi}
    print("modulation_spectrum (bank on the device): median %.3f ms (min %.3f max %.3f)" % (med, lo, hi))

    med, lo, hi = timed(lambda: metrics.msd(mels, mels_b, K, n_fft), a.warmup, a.iters)
    res["msd_ms"] = {"median": med, "min": lo, "max": hi}
    print("msd (two sets of host log-mels in, floats out: uploads, 2 projections, %d launches, read-back): median %.3f ms (min %.3f max %.3f)"
          % (res["launches_msd"], med, lo, hi))

    L = _hip.lib()
    table = _hip.device_constant(("metrics.ms_table", n_fft), cep.device, lambda: metrics.host_ms_table(n_fft))
    offs_d = torch.from_numpy(offs).cuda()
    power = torch.empty(a.utts, K, nb, dtype=torch.float32, device="cuda")
    mean = torch.empty(a.utts, K, dtype=torch.float32, device="cuda")
    var = torch.empty(a.utts, K, dtype=torch.float32, device="cuda")

    def raw():
        _hip.check(L.mcvc_ms_power(_hip.ptr(cep), cep.shape[1], K, _hip.ptr(offs_d), a.utts, offs.ctypes.data, n_fft, _hip.ptr(table), _hip.ptr(power),
                                   _hip.ptr(mean), _hip.ptr(var), _hip.stream()), "mcvc_ms_power")
    med, lo, hi = timed(raw, a.warmup, a.iters, inner=50)
    res["ms_power_kernel_ms"] = {"median": med, "min": lo, "max": hi, "launches_per_window": 50, "workgroups": a.utts * nb // 128,
                                 "tflops": flop / med / 1e9, "tflops_issued": flop_tiles / med / 1e9}
    print("ms_power alone, 50 launches per window: median %.4f ms per launch (min %.4f max %.4f) = %.1f TFLOP/s useful, %.1f TFLOP/s issued, %d workgroups"
          % (med, lo, hi, flop / med / 1e9, flop_tiles / med / 1e9, a.utts * nb // 128))
    lms = torch.empty(K, nb, dtype=torch.float32, device="cuda")

    def raw_log():
        _hip.check(L.mcvc_ms_mean_log(_hip.ptr(power), a.utts, K * nb, metrics.MS_FLOOR, _hip.ptr(lms), _hip.stream()), "mcvc_ms_mean_log")
    med, lo, hi = timed(raw_log, a.warmup, a.iters, inner=50)
    res["ms_mean_log_kernel_ms"] = {"median": med, "min": lo, "max": hi, "launches_per_window": 50}
    print("ms_mean_log alone ([%d, %d]): median %.4f ms per launch" % (a.utts, K * nb, med))
    per, tot = torch.empty(K, dtype=torch.float32, device="cuda"), torch.empty(1, dtype=torch.float32, device="cuda")

    def raw_dist():
        _hip.check(L.mcvc_ms_distance(_hip.ptr(lms), _hip.ptr(lms), K, nb, nb, _hip.ptr(per), _hip.ptr(tot), _hip.stream()), "mcvc_ms_distance")
    med, lo, hi = timed(raw_dist, a.warmup, a.iters, inner=50)
    res["ms_distance_kernel_ms"] = {"median": med, "min": lo, "max": hi, "launches_per_window": 50}
    print("ms_distance alone ([%d, %d]): median %.4f ms per launch" % (K, nb, med))

    # the yardstick: the library FFT of the zero-padded, mean-removed bank on the same device (buffers made once)
    padded = torch.zeros(a.utts, K, n_fft, dtype=torch.float32, device="cuda")
    for u, c in enumerate(metrics.split(cep, offs)):
        padded[u, :, :c.shape[1]] = c - c.mean(dim=1, keepdim=True)
    lens = torch.from_numpy(np.asarray(frames, dtype=np.float32)).cuda()[:, None, None]

    def fft():
        X = torch.fft.rfft(padded, dim=2)[:, :, 1:]
        return (X.real * X.real + X.imag * X.imag) / lens
    med, lo, hi = timed(fft, a.warmup, a.iters, inner=50)
    res["torch_rfft_power_ms"] = {"median": med, "min": lo, "max": hi, "launches_per_window": 50}
    print("torch.fft.rfft of the padded bank + |X|^2 / T (padding not timed): median %.4f ms per call (min %.4f max %.4f)" % (med, lo, hi))
    raw()
    torch.cuda.synchronize()
    ref = fft()
    rel = float(((power - ref).abs().max() / ref.abs().max()).cpu())
    res["largest_difference_to_torch_rfft_over_largest_power"] = rel
    print("largest |P - P_rfft| / largest P: %.2e" % rel)

    ceps = [c.cpu().numpy() for c in metrics.split(cep, offs)]
    t0 = time.perf_counter()
    ck.tables(ceps, n_fft)
    dt = time.perf_counter() - t0
    res["checker_cpu_s"] = dt
    print("float64 checker on the CPU (numpy rfft, one set of %d utterances): %.3f s" % (a.utts, dt))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
