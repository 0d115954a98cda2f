"""Checker of the wav -> log-mel front-end, shared by test_host_audio.py and test_hip_audio.py: a literal restatement of the five
steps of the transform with ``torch.stft`` on the CPU.  In float64 it is the truth; in float32 it is the reference's own arithmetic
(the MelGAN Audio2Mel module runs torch.stft in float32).  Nothing here comes from the code under test."""
import math

import numpy as np
import torch

N_FFT, HOP, N_MEL, RATE = 1024, 256, 80, 22050


def slaney_mel_basis():
    """float64 [80, 513]: librosa.filters.mel(sr=22050, n_fft=1024, n_mels=80, fmin=0, fmax=11025, htk=False, norm='slaney') by its
    definition, written with scalar loops so that it shares no code with the product's vectorised version."""
    def mel_to_hz(m):
        return 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0)) if m >= 15.0 else m * (200.0 / 3.0)
    top = 15.0 + math.log(11025.0 / 1000.0) / (math.log(6.4) / 27.0)
    e = [mel_to_hz(top * i / (N_MEL + 1)) for i in range(N_MEL + 2)]
    f = np.linspace(0.0, 11025.0, N_FFT // 2 + 1)
    B = np.zeros((N_MEL, N_FFT // 2 + 1), dtype=np.float64)
    for i in range(N_MEL):
        for b, fb in enumerate(f):
            B[i, b] = max(0.0, min((fb - e[i]) / (e[i + 1] - e[i]), (e[i + 2] - fb) / (e[i + 2] - e[i + 1]))) * 2.0 / (e[i + 2] - e[i])
    return B


_BASIS = slaney_mel_basis()


def log_mel(x, dtype=torch.float64):
    """One mono waveform (1-D array) -> [80, T] in ``dtype`` arithmetic; raises below 385 samples as torch's reflect padding does."""
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    p = (N_FFT - HOP) // 2
    xp = torch.nn.functional.pad(x[None, None], (p, p), "reflect")[0, 0]
    spec = torch.stft(xp, n_fft=N_FFT, hop_length=HOP, win_length=N_FFT, window=torch.hann_window(N_FFT, dtype=dtype), center=False,
                      return_complex=True)
    mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2)
    mel = torch.from_numpy(_BASIS).to(dtype) @ mag
    return torch.log10(torch.clamp(mel, min=1e-5))


def distances(got, truth):
    """(max abs error in log10 units, whole-tensor rel-L2) of ``got`` against the float64 result."""
    got, truth = torch.as_tensor(np.asarray(got)).double(), torch.as_tensor(np.asarray(truth)).double()
    return float((got - truth).abs().max()), float((got - truth).norm() / max(float(truth.norm()), 1e-30))


MAX_ABS_FLOOR, REL_L2_FLOOR = 1e-4, 2e-6


def gates(x, truth=None):
    """The bounds for input ``x``: twice the float32 checker's own distance to the float64 result, with floors of 1e-4 (max abs, log10
    units) and 2e-6 (rel-L2).  -> (truth, max-abs gate, rel-L2 gate, the float32 checker's distances)."""
    truth = log_mel(x, torch.float64) if truth is None else truth
    ref32 = distances(log_mel(x, torch.float32), truth)
    return truth, max(MAX_ABS_FLOOR, 2 * ref32[0]), max(REL_L2_FLOOR, 2 * ref32[1]), ref32


def check(tag, got, x):
    """Assert shape, finiteness and both gates of one utterance; prints the figures first."""
    truth, g_abs, g_rel, ref32 = gates(x)
    assert tuple(got.shape) == tuple(truth.shape), (tag, tuple(got.shape), tuple(truth.shape))
    assert np.isfinite(np.asarray(got)).all(), tag
    d = distances(got, truth)
    print("%-34s T %4d  max abs %.3e (gate %.3e, f32 checker %.3e)  rel-L2 %.3e (gate %.3e, f32 checker %.3e)"
          % (tag, truth.shape[1], d[0], g_abs, ref32[0], d[1], g_rel, ref32[1]))
    assert d[0] <= g_abs, (tag, "max abs", d[0], g_abs)
    assert d[1] <= g_rel, (tag, "rel-L2", d[1], g_rel)
    return truth
