"""Time of the HIP MelGAN decoder (csrc/vocoder_kernels.hip, MelVocoder.inverse) at the inference shapes, HIP events around whole
decodes after a warm-up; beside it the float32 torch restatement of the same network (tests/vocoder_checker.py, weight norm recomputed
per call as torch does) on the same GPU.  Synthetic weights: timing does not depend on their values.

    python tools/voc_bench.py [--iters 10] [--warmup 3] [--shapes 16x512,1x224]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "maskcyclegan-vc_amd"), os.path.join(ROOT, "tests")]

import vocoder_checker as ck  # noqa: E402
from mask_cyclegan_vc import _hip  # noqa: E402
from mask_cyclegan_vc.vocoder import MelVocoder, layer_table  # noqa: E402

PEAK_TFLOPS = 157.3                                          # fp32 MFMA peak the project's roofline uses


def flop_per_frame():
    """2 x multiply-adds of the 42 layers per mel frame (the time axis grows 8, 8, 2, 2-fold; a transposed conv of stride r and
    2r taps does 2 taps per output sample)."""
    total, up = 0.0, 1
    for name, shape in layer_table():
        if name in ("3", "8", "13", "18"):
            cin, cout, k = shape
            total += 2.0 * cin * cout * k * up               # per INPUT sample: k taps x Cout outputs
            up *= k // 2
        else:
            cout, cin, k = shape
            total += 2.0 * cin * cout * k * up
    return total


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
    ap.add_argument("--shapes", type=str, default="16x512,1x224")
    a = ap.parse_args()
    voc = MelVocoder().load_state_dict(ck.state_dict())
    ref = ck.synthetic_generator().cuda()
    launches = _hip.lib().mcvc_voc_launches()
    per_frame = flop_per_frame()
    print("MelGAN decoder: %.1f MFLOP per mel frame, %d launches per decode" % (per_frame / 1e6, launches))
    for shape in a.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        mel = ck.synthetic_mel(B, T, 1).cuda()
        flop = per_frame * B * T
        med, lo, hi = timed(lambda: voc.inverse(mel), a.warmup, a.iters)
        with torch.no_grad():
            t_med, t_lo, t_hi = timed(lambda: ref(mel), a.warmup, a.iters)
            diff = float((voc.inverse(mel) - ref(mel).squeeze(1)).abs().max())
        print("B=%d T=%d (%.1f GFLOP): HIP decode median %.3f ms (min %.3f max %.3f) = %.1f TFLOP/s, %.1f %% of the %.1f TF/s fp32 MFMA peak | "
              "torch float32 restatement on this GPU median %.3f ms (min %.3f max %.3f) = %.2fx the HIP decode | max |HIP - torch| %.2e"
              % (B, T, flop / 1e9, med, lo, hi, flop / med / 1e9, 100.0 * flop / med / 1e9 / PEAK_TFLOPS, PEAK_TFLOPS, t_med, t_lo, t_hi, t_med / med, diff))


if __name__ == "__main__":
    main()
