"""Time of the batched HIP DTW (csrc/dtw_kernels.hip, mask_cyclegan_vc.metrics.dtw) on a VCC2018-like evaluation set: 35 pairs with
lengths spread over 150 .. 900 frames, K = 24, with and without paths; HIP events around whole batched calls after a warm-up (table
upload and output allocation included: what a caller pays).  Beside it the kernels alone through the C ABI on buffers made once, the
cepstra projection of the same set, and the CPU time of the float64 checker (tests/dtw_checker.py, the plain double loop) for ONE pair.
Informational, not a gate: there is nothing older to compare against.

    python tools/dtw_bench.py [--iters 10] [--warmup 3] [--pairs 35] [--k 24] [--checker_frames 300]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "maskcyclegan-vc_amd"), os.path.join(ROOT, "tests")]

import dtw_checker as ck  # noqa: E402
from mask_cyclegan_vc import _hip, metrics  # noqa: E402


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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=35)
    ap.add_argument("--k", type=int, default=24)
    ap.add_argument("--checker_frames", type=int, default=300)
    a = ap.parse_args()
    rs = np.random.RandomState(0)
    tx = rs.randint(150, 901, size=a.pairs)
    ty = np.clip((tx * rs.uniform(0.8, 1.25, size=a.pairs)).astype(int), 150, 900)
    xs = [rs.randn(a.k, int(t)).astype(np.float32) for t in tx]
    ys = [rs.randn(a.k, int(t)).astype(np.float32) for t in ty]
    xb, xo = metrics.bank(xs)
    yb, yo = metrics.bank(ys)
    cells = float((tx * ty).sum())
    strips = (tx + 63) // 64
    print("%d pairs, K = %d: Tx %d .. %d, Ty %d .. %d, %.2f M cells; the longest pair sweeps %d strips x (Ty + 63) = %d dependent steps"
          % (a.pairs, a.k, tx.min(), tx.max(), ty.min(), ty.max(), cells / 1e6, int(strips.max()), int((strips * (ty + 63)).max())))
    L = _hip.lib()
    for want_path in (False, True):
        med, lo, hi = timed(lambda: metrics.dtw((xb, xo), (yb, yo), metrics.MCD_SCALE, return_path=want_path), a.warmup, a.iters)
        table, ws_bytes, rows = metrics.plan(xo, yo, want_path)
        td = torch.from_numpy(table).cuda()
        cost = torch.empty(a.pairs, dtype=torch.float32, device="cuda")
        length = torch.empty(a.pairs, dtype=torch.int32, device="cuda")
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
        path = torch.empty(max(rows, 1), 2, dtype=torch.int32, device="cuda") if want_path else None

        def raw():
            _hip.check(L.mcvc_dtw_run(_hip.ptr(xb), xb.shape[1], _hip.ptr(yb), yb.shape[1], a.k, metrics.MCD_SCALE, xo.ctypes.data, yo.ctypes.data,
                                      _hip.ptr(td), a.pairs, _hip.ptr(cost), _hip.ptr(length), _hip.ptr(path), _hip.ptr(ws), ws_bytes, _hip.stream()),
                       "mcvc_dtw_run")
        kmed, klo, khi = timed(raw, a.warmup, a.iters)
        print("paths %-5s: metrics.dtw median %.3f ms (min %.3f max %.3f) | kernels alone (%d launch%s) median %.3f ms (min %.3f max %.3f) = "
              "%.2f G cells/s | workspace %.2f MB" % (want_path, med, lo, hi, L.mcvc_dtw_launches(int(want_path)), "es" if want_path else "", kmed, klo, khi,
                                                      cells / kmed / 1e6, ws_bytes / 1e6))
    mels = [(-2.0 + rs.randn(80, int(t))).astype(np.float32) for t in tx]
    mb = metrics.bank(mels)
    med, lo, hi = timed(lambda: metrics.mel_cepstra(mb, a.k if a.k < 80 else 24), a.warmup, a.iters)
    print("mel_cepstra of the %d frames of one side: median %.3f ms (min %.3f max %.3f)" % (int(tx.sum()), med, lo, hi))
    T = a.checker_frames
    t0 = time.perf_counter()
    c64, n64, _ = ck.dtw(xs[0][:, :T], ys[0][:, :T], metrics.MCD_SCALE)
    dt = time.perf_counter() - t0
    c, n = metrics.dtw([xs[0][:, :T]], [ys[0][:, :T]], metrics.MCD_SCALE)
    print("float64 checker on the CPU, ONE pair of %d x %d frames: %.2f s = %.1f us per cell (the whole set at that rate: %.0f s); HIP cost %.6g against %.9g, "
          "length %d against %d" % (T, T, dt, dt / (T * T) * 1e6, dt / (T * T) * cells, float(c[0]), c64, int(n[0]), n64))


if __name__ == "__main__":
    main()
