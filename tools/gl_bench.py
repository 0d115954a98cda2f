"""Time of the HIP Griffin-Lim decoder (csrc/griffinlim_kernels.hip, GriffinLimVocoder.inverse) at the inference shapes, HIP events
around whole decodes after a warm-up; beside it a float32 torch restatement of the same iteration on the same GPU (torch.stft,
irfft, overlap-add by F.fold), checked here against tests/griffinlim_checker.py at a small shape.  Informational, not a gate.

    python tools/gl_bench.py [--iters 5] [--warmup 2] [--shapes 16x512,1x224] [--n_iter 32]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "maskcyclegan-vc_amd"), os.path.join(ROOT, "tests")]

import griffinlim_checker as ck  # noqa: E402
from mask_cyclegan_vc import _hip  # noqa: E402
from mask_cyclegan_vc.griffinlim import GriffinLimVocoder  # noqa: E402

PEAK_TFLOPS = 157.3                                          # fp32 MFMA peak the project's roofline uses
N, HOP, PAD = 1024, 256, 384
FLOP_PER_FRAME_DIRECTION = 2.0 * N * N                       # a dense 1024-point real DFT as a matrix product


def torch_griffin_lim(logmel, angles, n_iter, momentum, pinv):
    """The iteration in float32 torch ops on the device of ``logmel`` ([B, 80, T]); angles (re, im) [B, 513, T, 2]."""
    Bn, _, T = logmel.shape
    w = torch.hann_window(N, dtype=torch.float32, device=logmel.device)
    L = HOP * (T - 1) + N
    env = torch.nn.functional.fold((w * w)[None, :, None].expand(1, N, T), (1, L), (1, N), stride=(1, HOP))[0, 0, 0, PAD:PAD + HOP * T]

    def istft(S):
        frames = torch.fft.irfft(S, n=N, dim=1) * w[None, :, None]
        return torch.nn.functional.fold(frames, (1, L), (1, N), stride=(1, HOP))[:, 0, 0, PAD:PAD + HOP * T] / env

    def stft(x):
        xp = torch.nn.functional.pad(x[:, None, :], (PAD, PAD), "reflect")[:, 0]
        return torch.stft(xp, n_fft=N, hop_length=HOP, win_length=N, window=w, center=False, return_complex=True)

    M = torch.clamp(pinv @ (10.0 ** logmel), min=0.0)
    A = torch.complex(angles[..., 0].contiguous(), angles[..., 1].contiguous())
    R_prev = torch.zeros_like(A)
    c = momentum / (1.0 + momentum)
    for _ in range(n_iter):
        R = stft(istft(M * A))
        Z = R - c * R_prev
        A = Z / (Z.abs() + 1e-16)
        R_prev = R
    return istft(M * A)


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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", type=str, default="16x512,1x224")
    ap.add_argument("--n_iter", type=int, default=32)
    a = ap.parse_args()
    gl = GriffinLimVocoder(n_iter=a.n_iter)
    pinv = torch.from_numpy(ck.pinv_basis().astype(np.float32)).cuda()
    rs = np.random.RandomState(0)
    small = torch.from_numpy((-2.0 + rs.randn(1, 80, 9)).astype(np.float32)).cuda()
    ang = gl.angles(1, 9)
    want = ck.griffin_lim(ck.magnitude_from_mel(small.cpu().numpy()), ang.cpu().numpy(), 2, 0.99)
    d = ck.distances(torch_griffin_lim(small, ang, 2, 0.99, pinv).cpu().numpy(), want)
    print("torch restatement against the float64 checker at 1x9, 2 iterations: rel-L2 %.2e, max / peak %.2e" % d)
    assert d[0] < 1e-4, "the restatement timed here is not the transform"
    print("Griffin-Lim decoder: %.2f MFLOP per frame and direction, %d launches per decode of %d iterations"
          % (FLOP_PER_FRAME_DIRECTION / 1e6, _hip.lib().mcvc_gl_launches(a.n_iter), a.n_iter))
    for shape in a.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        mel = torch.from_numpy((-2.0 + rs.randn(B, 80, T)).astype(np.float32)).cuda()
        ang = gl.angles(B, T)
        flop = FLOP_PER_FRAME_DIRECTION * B * T * (2 * a.n_iter + 1)
        med, lo, hi = timed(lambda: gl.inverse(mel, angles=ang), a.warmup, a.iters)
        with torch.no_grad():
            t_med, t_lo, t_hi = timed(lambda: torch_griffin_lim(mel, ang, a.n_iter, gl.momentum, pinv), a.warmup, a.iters)
        print("B=%d T=%d n_iter=%d (%.1f GFLOP as dense products): HIP decode median %.3f ms (min %.3f max %.3f) = %.1f TFLOP/s, %.1f %% of the "
              "%.1f TF/s fp32 MFMA peak | torch float32 restatement (FFT) on this GPU median %.3f ms (min %.3f max %.3f) = %.2fx the HIP decode"
              % (B, T, a.n_iter, flop / 1e9, med, lo, hi, flop / med / 1e9, 100.0 * flop / med / 1e9 / PEAK_TFLOPS, PEAK_TFLOPS, t_med, t_lo, t_hi,
                 t_med / med))


if __name__ == "__main__":
    main()
