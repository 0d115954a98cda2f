"""Time of the HIP silence detector (csrc/vad_kernels.hip, data_preprocessing.silence.SilenceDetector) on two banks:

  utterances   the evaluation set the other tools use: 35 utterances of 150 .. 900 mel frames (256 samples each);
  recording    one 10-minute recording, 13.2 M samples: a single utterance.

Per bank, after a warm-up, in alternating repeats (kernel, energies, kernel, energies, ...: a drift of the clocks shows as spread in both):
  kernel       mcvc_vad_energy alone (its memset node and its kernel) through the C ABI on buffers made once: HIP events around a window of
               back-to-back calls, divided by their number; GB/s over the bytes the algorithm needs, 4 samples + 4 (frames + utterances),
               and their share of the 6.3 TB/s a streaming kernel reaches on this chip (8 TB/s on paper).  Both banks (20 MB, 53 MB) fit the
               256 MiB Infinity Cache and the window reads the same buffer again and again: the rate is the warm-cache one, an upper bound
               on what a first pass over a freshly uploaded bank sees;
  energies     SilenceDetector.energies from host waveforms to host arrays (upload, plan, launch, download): host clock around a call that
               ends in a synchronising copy;
  numpy        the same energies restated in numpy float32 on this host (512-sample block sums, four blocks per frame).
Informational, not a gate: there is nothing older to compare against.  Writes profiles/vad_bench.json.

    python tools/vad_bench.py [--iters 20] [--warmup 5] [--window 2000] [--utts 35] [--out profiles/vad_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "maskcyclegan-vc_amd")]

HBM_STREAM_TBPS, HBM_PEAK_TBPS = 6.3, 8.0


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def numpy_energies(waves):
    """The definition in numpy float32: block sums of squares, a frame = its four blocks."""
    out = []
    for w in waves:
        T = 1 + w.size // 512
        sq = np.zeros(512 * (T + 3), dtype=np.float32)
        sq[1024:1024 + w.size] = w * w
        b = sq.reshape(T + 3, 512).sum(axis=1, dtype=np.float32)
        m = (b[0:T] + b[1:T + 1] + b[2:T + 2] + b[3:T + 3]) * np.float32(1.0 / 2048)
        out.append((m, m.max()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=int, default=2000, help="back-to-back calls per timed window (tens of milliseconds per window)")
    ap.add_argument("--utts", type=int, default=35)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "vad_bench.json"))
    a = ap.parse_args()
    import torch
    from data_preprocessing.silence import SilenceDetector
    from mask_cyclegan_vc import _hip
    if not torch.cuda.is_available():
        raise SystemExit("vad_bench needs a HIP device: a time taken anywhere else says nothing about the kernel")
    L = _hip.lib()
    rng = np.random.RandomState(0)
    frames = rng.randint(150, 901, size=a.utts)
    det = SilenceDetector()
    banks = {"utterances": [(0.1 * rng.randn(256 * int(t))).astype(np.float32) for t in frames],
             "recording": [(0.1 * rng.randn(600 * 22050)).astype(np.float32)]}
    result = {"iters": a.iters, "window": a.window, "device": torch.cuda.get_device_name(0), "tile_frames": L.mcvc_vad_tile_frames(),
              "launches_per_call": L.mcvc_vad_launches(), "hbm_stream_TBps": HBM_STREAM_TBPS, "hbm_peak_TBps": HBM_PEAK_TBPS,
              "note": "back-to-back calls over one buffer that fits the 256 MiB Infinity Cache: warm-cache rates, not a cold pass from HBM", "cases": {}}
    for name, waves in banks.items():
        n = len(waves)
        lengths = [w.size for w in waves]
        total = int(sum(lengths))
        offs = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(lengths, out=offs[1:])
        fo = np.zeros(n + 1, dtype=np.int32)
        nt = ctypes.c_int(0)
        _hip.check(L.mcvc_vad_plan(offs.ctypes.data, n, fo.ctypes.data, None, 0, ctypes.byref(nt)), "mcvc_vad_plan")
        tiles = np.zeros((nt.value, 4), dtype=np.int32)
        _hip.check(L.mcvc_vad_plan(offs.ctypes.data, n, fo.ctypes.data, tiles.ctypes.data, nt.value, ctypes.byref(nt)), "mcvc_vad_plan")
        n_frames = int(fo[-1])
        wave = torch.from_numpy(np.concatenate(waves)).cuda()
        tiles_d, fo_d = torch.from_numpy(tiles).cuda(), torch.from_numpy(fo).cuda()
        mse = torch.empty(n_frames, dtype=torch.float32, device="cuda")
        ref = torch.empty(n, dtype=torch.float32, device="cuda")

        def raw():
            _hip.check(L.mcvc_vad_energy(_hip.ptr(wave), total, _hip.ptr(tiles_d), nt.value, _hip.ptr(fo_d), n, _hip.ptr(mse), n_frames, _hip.ptr(ref),
                                         _hip.stream()), "mcvc_vad_energy")
        for _ in range(a.warmup):
            raw()
            det.energies(waves)
        torch.cuda.synchronize()
        kernel_us, whole_ms = [], []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.window):
                raw()
            e1.record()
            torch.cuda.synchronize()
            kernel_us.append(1e3 * e0.elapsed_time(e1) / a.window)
            t0 = time.perf_counter()
            det.energies(waves)                                        # ends in the copy of the energies to the host
            whole_ms.append(1e3 * (time.perf_counter() - t0))
        host_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            numpy_energies(waves)
            host_ms.append(1e3 * (time.perf_counter() - t0))
        k = median(kernel_us)
        nbytes = 4.0 * total + 4.0 * (n_frames + n)
        gbps = nbytes / k / 1e3
        case = {"utterances": n, "samples": total, "frames": n_frames, "workgroups": nt.value,
                "bytes": {"samples_read": 4.0 * total, "mse_written": 4.0 * n_frames, "ref_written": 4.0 * n},
                "kernel_us_median": round(k, 2), "kernel_us_min": round(min(kernel_us), 2), "kernel_us_max": round(max(kernel_us), 2),
                "achieved_GBps": round(gbps, 1), "share_of_hbm_stream": round(gbps / (1e3 * HBM_STREAM_TBPS), 4),
                "share_of_hbm_peak": round(gbps / (1e3 * HBM_PEAK_TBPS), 4),
                "energies_ms_median": round(median(whole_ms), 3), "energies_ms_min": round(min(whole_ms), 3), "energies_ms_max": round(max(whole_ms), 3),
                "numpy_float32_host_ms_median": round(median(host_ms), 2)}
        result["cases"][name] = case
        print("%s: %d utterances, %d samples, %d frames, %d workgroups; call median %.1f us (min %.1f max %.1f) = %.0f GB/s = %.1f %% of %.1f TB/s; "
              "energies() host to host median %.2f ms (min %.2f max %.2f); numpy float32 on the host %.1f ms"
              % (name, n, total, n_frames, nt.value, k, min(kernel_us), max(kernel_us), gbps, 100.0 * gbps / (1e3 * HBM_STREAM_TBPS), HBM_STREAM_TBPS,
                 median(whole_ms), min(whole_ms), max(whole_ms), median(host_ms)))
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
