"""Time of the HIP resampler (csrc/resample_kernels.hip, data_preprocessing.resample.Resampler) on the evaluation set the other tools use: 35
utterances of 150 .. 900 frames (their length at 22050 Hz), recorded at 48000 Hz and at 16000 Hz and brought to 22050 Hz.

Per rate, after a warm-up, medians over repetitions:
  kernel       the launch alone through the C ABI on buffers made once: HIP events around a window of back-to-back launches, divided by
               their number (one launch of some tens of microseconds is shorter than an event pair resolves well); GB/s over the bytes the
               algorithm needs, 4 (n_in + n_out), against which a streaming kernel is judged;
  bank_at_rates  the whole Audio2Mel.bank_at_rates call from host waveforms to host mels (upload, plan, resample, log-mel, download),
               host clock around a call that ends in a synchronising copy;
  scipy        scipy.signal.resample_poly in float64 over the same files on this host, one at a time: what read_wav does today.
Informational, not a gate: there is nothing older to compare against.  Writes profiles/resample_bench.json.

    python tools/resample_bench.py [--iters 30] [--warmup 5] [--window 50] [--utts 35] [--out profiles/resample_bench.json]
    python tools/resample_bench.py --banks      # no GPU: LDS bank conflicts of the table reads per half-wave, natural against odd row pitch
"""
import argparse
import ctypes
import json
import os
import sys
import time
from math import gcd

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "maskcyclegan-vc_amd")]

RATES = (8000, 11025, 12000, 16000, 24000, 32000, 44100, 48000, 88200, 96000)


def worst_conflict(up, down, pitch):
    """Largest number of DIFFERENT table words that one bank serves in one 32-lane half of a full row's ds_read (same word: a broadcast)."""
    worst = 0
    for r0 in range(min(up, 8)):
        i = np.arange(1024)
        r = (r0 + i * down) % up
        for h in range(0, 1024, 32):
            words = {}
            for a in r[h:h + 32] * pitch:
                words.setdefault(int(a) % 32, set()).add(int(a))
            worst = max(worst, max(len(v) for v in words.values()))
    return worst


def banks():
    print("rate pair          up/down   J   natural pitch J   odd pitch J|1")
    for rate in RATES:
        for a, b in ((rate, 22050), (22050, rate)):
            g = gcd(a, b)
            up, down = b // g, a // g
            J = -(-(20 * max(up, down) + 1) // up)
            print("%6d -> %6d  %3d/%-3d  %4d   %d-way             %d-way" % (a, b, up, down, J, worst_conflict(up, down, J), worst_conflict(up, down, J | 1)))


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=int, default=50, help="back-to-back launches per timed window")
    ap.add_argument("--utts", type=int, default=35)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    ap.add_argument("--banks", action="store_true")
    a = ap.parse_args()
    if a.banks:
        return banks()
    import torch
    from scipy.signal import resample_poly
    from data_preprocessing.audio2mel import Audio2Mel
    from data_preprocessing.resample import Resampler, ratio
    from mask_cyclegan_vc import _hip
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs a HIP device: a time taken anywhere else says nothing about the kernel")
    L = _hip.lib()
    rng = np.random.RandomState(0)
    frames = rng.randint(150, 901, size=a.utts)
    rs, fft = Resampler(), Audio2Mel()
    result = {"utterances": int(a.utts), "frames_at_22050": [int(frames.min()), int(frames.max())], "iters": a.iters, "window": a.window,
              "device": torch.cuda.get_device_name(0), "cases": {}}
    for rate in (48000, 16000):
        up, down = ratio(rate, 22050)
        lengths = [int(256 * t * down // up) for t in frames]
        waves = [(0.1 * rng.randn(n)).astype(np.float32) for n in lengths]
        n_in = int(sum(lengths))
        offs = np.zeros(a.utts + 1, dtype=np.int32)
        np.cumsum(lengths, out=offs[1:])
        oo = np.zeros(a.utts + 1, dtype=np.int32)
        nt = ctypes.c_int(0)
        _hip.check(L.mcvc_resample_plan(offs.ctypes.data, a.utts, up, down, oo.ctypes.data, None, 0, ctypes.byref(nt)), "mcvc_resample_plan")
        tiles = torch.zeros(nt.value, 8, dtype=torch.int32).pin_memory()
        _hip.check(L.mcvc_resample_plan(offs.ctypes.data, a.utts, up, down, oo.ctypes.data, tiles.data_ptr(), nt.value, ctypes.byref(nt)), "mcvc_resample_plan")
        n_out = int(oo[-1])
        wave = torch.from_numpy(np.concatenate(waves)).cuda()
        out = torch.empty(n_out, dtype=torch.float32, device="cuda")
        table = rs.table(up, down)

        def raw():
            _hip.check(L.mcvc_resample_run(_hip.ptr(wave), n_in, ctypes.c_void_p(tiles.data_ptr()), nt.value, _hip.ptr(table), up, down, _hip.ptr(out),
                                           n_out, _hip.stream()), "mcvc_resample_run")
        for _ in range(a.warmup):
            raw()
        torch.cuda.synchronize()
        kernel_us = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.window):
                raw()
            e1.record()
            torch.cuda.synchronize()
            kernel_us.append(1e3 * e0.elapsed_time(e1) / a.window)
        k = median(kernel_us)
        nbytes = 4.0 * (n_in + n_out)
        rates = [rate] * a.utts
        for _ in range(a.warmup):
            fft.bank_at_rates(waves, rates)
        whole_ms = []
        for _ in range(a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fft.bank_at_rates(waves, rates)                            # ends in the copy of the mels to the host
            whole_ms.append(1e3 * (time.perf_counter() - t0))
        host_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            for w in waves:
                resample_poly(w.astype(np.float64), up, down)
            host_ms.append(1e3 * (time.perf_counter() - t0))
        case = {"up": up, "down": down, "samples_in": n_in, "samples_out": n_out, "workgroups": nt.value,
                "kernel_us_median": round(k, 2), "kernel_us_min": round(min(kernel_us), 2), "kernel_us_max": round(max(kernel_us), 2),
                "bytes_in_plus_out": nbytes, "achieved_GBps": round(nbytes / k / 1e3, 1),
                "bank_at_rates_ms_median": round(median(whole_ms), 3), "bank_at_rates_ms_min": round(min(whole_ms), 3),
                "scipy_resample_poly_host_ms_median": round(median(host_ms), 1)}
        result["cases"]["%d->22050" % rate] = case
        print("%d -> 22050 Hz (%d/%d): %d -> %d samples, %d workgroups; kernel median %.1f us (min %.1f max %.1f) = %.0f GB/s over in + out bytes; "
              "bank_at_rates (host waveforms -> host mels) median %.2f ms; scipy.resample_poly on the host %.0f ms"
              % (rate, up, down, n_in, n_out, nt.value, k, min(kernel_us), max(kernel_us), nbytes / k / 1e3, median(whole_ms), median(host_ms)))
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
