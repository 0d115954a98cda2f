"""Checker of the Griffin-Lim decoder, shared by test_host_griffinlim.py, test_hip_griffinlim.py and tools/gl_bench.py: a literal
restatement of the transform with ``torch.stft`` / ``torch.fft.irfft`` -- float64 is the truth, float32 the yardstick.  Nothing here
comes from the code under test.

    M = max(0, pinv(B) @ 10**logmel)                      B = audio_checker.slaney_mel_basis(), pinv by numpy.linalg.pinv in float64
    STFT(x):  reflect-pad 384, torch.stft(center=False) with the periodic Hann window w, n_fft 1024, hop 256
    ISTFT(S): frame_t = w * irfft(S[:, t], 1024);  y[p] = sum_t frame_t[p - 256 t] / sum_t w^2[p - 256 t];  keep p in [384, 384 + 256 T)
              (an explicit overlap-add loop: torch.istft refuses this framing because w[0] = 0)
    A_0 given, R_-1 = 0;  k < n_iter:  R_k = STFT(ISTFT(M A_k)),  Z = R_k - m / (1 + m) R_k-1,  A_k+1 = Z / (|Z| + 1e-16)
    result = ISTFT(M A_n_iter)
"""
import numpy as np
import torch

import audio_checker as ack

N_FFT, HOP, N_MEL, N_BIN = ack.N_FFT, ack.HOP, ack.N_MEL, ack.N_FFT // 2 + 1
PAD = (N_FFT - HOP) // 2
FLOOR = 2e-6                                                # both distances; from CPU measurements of the float32 checker, not from the kernel

_PINV = np.linalg.pinv(ack.slaney_mel_basis())              # float64 [513, 80]


def pinv_basis():
    return _PINV.copy()


def _cdtype(dtype):
    return torch.complex128 if dtype == torch.float64 else torch.complex64


def window(dtype):
    return torch.hann_window(N_FFT, dtype=dtype)


def stft(x, dtype=torch.float64):
    """[B, 256 T] -> complex [B, 513, T]."""
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    xp = torch.nn.functional.pad(x[:, None, :], (PAD, PAD), "reflect")[:, 0]
    return torch.stft(xp, n_fft=N_FFT, hop_length=HOP, win_length=N_FFT, window=window(dtype), center=False, return_complex=True)


def istft(S, dtype=torch.float64):
    """complex [B, 513, T] -> [B, 256 T]; the imaginary parts of bins 0 and 512 are ignored, as irfft ignores them."""
    S = torch.as_tensor(S).to(_cdtype(dtype))
    Bn, _, T = S.shape
    w = window(dtype)
    frames = torch.fft.irfft(S, n=N_FFT, dim=1) * w[None, :, None]       # [B, 1024, T]
    y = torch.zeros(Bn, HOP * (T - 1) + N_FFT, dtype=dtype)
    env = torch.zeros(HOP * (T - 1) + N_FFT, dtype=dtype)
    for t in range(T):
        y[:, HOP * t:HOP * t + N_FFT] += frames[:, :, t]
        env[HOP * t:HOP * t + N_FFT] += w * w
    keep = slice(PAD, PAD + HOP * T)
    return y[:, keep] / env[keep]


def magnitude_from_mel(logmel, dtype=torch.float64):
    """log10-mel [B, 80, T] -> [B, 513, T]."""
    logmel = torch.as_tensor(np.asarray(logmel)).to(dtype)
    return torch.clamp(torch.from_numpy(_PINV).to(dtype) @ (10.0 ** logmel), min=0.0)


def to_complex(angles, dtype=torch.float64):
    """(re, im) [B, 513, T, 2] -> complex [B, 513, T] in ``dtype`` arithmetic."""
    a = torch.as_tensor(np.asarray(angles)).to(dtype)
    return torch.complex(a[..., 0].contiguous(), a[..., 1].contiguous())


def griffin_lim(M, angles0, n_iter, momentum, dtype=torch.float64):
    """M [B, 513, T] (any real dtype), angles0 (re, im) [B, 513, T, 2] or None (zero phase) -> [B, 256 T] in ``dtype`` arithmetic."""
    M = torch.as_tensor(np.asarray(M)).to(dtype)
    A = torch.ones(M.shape, dtype=_cdtype(dtype)) if angles0 is None else to_complex(angles0, dtype)
    R_prev = torch.zeros(M.shape, dtype=_cdtype(dtype))
    c = momentum / (1.0 + momentum)
    for _ in range(n_iter):
        x = istft(M * A, dtype)
        R = stft(x, dtype)
        Z = R - c * R_prev
        A = Z / (Z.abs() + 1e-16)
        R_prev = R
    return istft(M * A, dtype)


def distances(got, truth):
    """(whole-tensor rel-L2, max abs error over the peak of the truth) against the float64 result."""
    got, truth = torch.as_tensor(np.asarray(got)).double(), torch.as_tensor(np.asarray(truth)).double()
    d = got - truth
    return float(d.norm() / max(float(truth.norm()), 1e-300)), float(d.abs().max() / max(float(truth.abs().max()), 1e-300))


def check(tag, got, truth, ref32, k):
    """Both distances of ``got`` within max(FLOOR, k x the float32 checker's own distance); prints the figures and ratios first.
    -> the larger of the two ratios (distance / gate)."""
    assert tuple(got.shape) == tuple(truth.shape), (tag, tuple(got.shape), tuple(truth.shape))
    assert np.isfinite(np.asarray(got)).all(), tag
    d, r = distances(got, truth), distances(ref32, truth)
    g = [max(FLOOR, k * v) for v in r]
    print("%-46s rel-L2 %.3e (gate %.3e, f32 checker %.3e, ratio to it %.2f)  max/peak %.3e (gate %.3e, f32 checker %.3e, ratio to it %.2f)"
          % (tag, d[0], g[0], r[0], d[0] / max(r[0], 1e-300), d[1], g[1], r[1], d[1] / max(r[1], 1e-300)))
    assert d[0] <= g[0], (tag, "rel-L2", d[0], g[0])
    assert d[1] <= g[1], (tag, "max abs / peak", d[1], g[1])
    return max(d[0] / g[0], d[1] / g[1])


def spectral_convergence(x, M):
    """|| |STFT(x)| - M || / || M ||, evaluated in float64."""
    M = torch.as_tensor(np.asarray(M)).double()
    return float((stft(x, torch.float64).abs() - M).norm() / M.norm())
