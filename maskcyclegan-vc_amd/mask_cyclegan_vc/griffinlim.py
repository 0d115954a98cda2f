"""Griffin-Lim decoder: log-mel (or linear magnitude) -> waveform on the HIP kernels, with the interface of ``MelVocoder`` and no
weights -- the audio path for a machine that has no MelGAN checkpoint.

* ``gl.inverse(mel)``         [B, 80, T] log10-mel -> [B, 256 T] float32 waveform (csrc/griffinlim_kernels.hip through ``mcvc_gl_decode``);
* ``gl.from_magnitude(mag)``  the same from a linear magnitude [B, 513, T] (non-negative);
* ``gl(audio)``               waveform -> log-mel, ``data_preprocessing.audio2mel.Audio2Mel``.
* ``GriffinLimVocoder(mel_inverse="nnls", mel_iter=64)``: ``inverse(mel)`` is ``from_magnitude(MelInverter(n_iter=mel_iter)(mel))`` -- the
  magnitude comes from the non-negative least-squares solver of ``mask_cyclegan_vc/melinv.py`` instead of the clamped pseudo-inverse
  below.  The default ``"pinv"`` changes nothing.

The transform is fixed by the front-end's STFT (reflect-pad 384, frames of 1024 at hop 256, periodic Hann w, bins 0..512):

    M = max(0, pinv(mel basis) @ 10**logmel)              pinv: numpy.linalg.pinv in float64, used as float32
    ISTFT(S): y[p] = sum_t (w irfft(S[:, t]))[p - 256 t] / sum_t w^2[p - 256 t], kept for p in [384, 384 + 256 T)
    A_0 unit modulus, R_-1 = 0;  k < n_iter:  R_k = STFT(ISTFT(M A_k)),  Z = R_k - m / (1 + m) R_k-1,  A_k+1 = Z / |Z|
    result = ISTFT(M A_n_iter)                            (fast Griffin-Lim, the form librosa and torchaudio use)

Initial angles.  No random numbers are drawn inside a kernel: ``angles(B, T)`` draws ``2 pi rand`` from a ``torch.Generator`` on the
device seeded with ``seed`` and takes cos / sin in torch.  The stream is restarted per sample, so every sample of a batch gets the
angles a single call of the same length gets: a batch equals its single calls, and two calls with the same seed and shape give the
same bits.  ``angles=`` overrides them: a float32 (re, im) tensor [B, 513, T, 2], or ``ZERO_PHASE``.

Quality is below MelGAN (Griffin-Lim from 80 mel bands sounds metallic); the decoder is deterministic, offline and checked against a
float64 restatement (tests/griffinlim_checker.py).  There is no CPU path.
"""
import math

import numpy as np
import torch

from . import _hip

N_MEL = 80
N_BIN = 513
HOP = 256
MIN_FRAMES = 2
ZERO_PHASE = "zero"
KIND_LOGMEL, KIND_LINEAR = 0, 1


def pinv_mel_basis():
    """float64 [513, 80]: the pseudo-inverse of the front-end's Slaney mel basis."""
    from data_preprocessing.audio2mel import mel_filterbank
    return np.linalg.pinv(mel_filterbank(np.float64))


def host_tables():
    """The decoder's constant operand as a float32 host array (``mcvc_gl_tables_init``)."""
    L = _hip.lib()
    pinv = np.ascontiguousarray(pinv_mel_basis(), dtype=np.float32)
    host = np.empty(L.mcvc_gl_tables_floats(), dtype=np.float32)
    _hip.check(L.mcvc_gl_tables_init(pinv.ctypes.data, host.ctypes.data), "mcvc_gl_tables_init")
    return host


class GriffinLimVocoder(object):
    """``GriffinLimVocoder(device=None, n_iter=32, momentum=0.99, seed=0, mel_inverse="pinv", mel_iter=64)``; then ``inverse(mel)``,
    ``from_magnitude(mag)`` and ``__call__(audio)``."""

    def __init__(self, device=None, n_iter=32, momentum=0.99, seed=0, mel_inverse="pinv", mel_iter=64):
        self.device = _hip.hip_device("mask_cyclegan_vc.griffinlim", device)
        if int(n_iter) < 0:
            raise ValueError("n_iter must be >= 0, got %r" % (n_iter,))
        if not 0.0 <= float(momentum) < 1.0:
            raise ValueError("momentum must lie in [0, 1), got %r" % (momentum,))
        self.n_iter, self.momentum, self.seed = int(n_iter), float(momentum), int(seed)
        self._fft = None
        if mel_inverse not in ("pinv", "nnls"):
            raise ValueError("mel_inverse is 'pinv' or 'nnls', got %r" % (mel_inverse,))
        self.mel_inverse, self._melinv = mel_inverse, None
        if mel_inverse == "nnls":
            from .melinv import MelInverter
            self._melinv = MelInverter(self.device, n_iter=mel_iter)

    def tables(self):
        return _hip.device_constant("griffinlim.tables", self.device, host_tables)

    def angles(self, B, T):
        """The initial angles of a [B, ., T] call as (re, im) float32 [B, 513, T, 2]: one seeded draw of [513, T], the same for every sample."""
        with torch.cuda.device(self.device):
            gen = torch.Generator(device=self.device)
            gen.manual_seed(self.seed)
            theta = (2.0 * math.pi) * torch.rand(N_BIN, T, generator=gen, device=self.device, dtype=torch.float32)
            one = torch.stack((torch.cos(theta), torch.sin(theta)), dim=-1)
            return one[None].expand(B, N_BIN, T, 2).contiguous()

    def _decode(self, x, kind, rows, angles, n_iter, momentum):
        _hip.require_on_device("mask_cyclegan_vc.griffinlim", x, self.device, "input", "decoder")
        if x.dim() != 3 or x.shape[1] != rows:
            raise ValueError("expected a [B, %d, T] tensor, got %s" % (rows, tuple(x.shape)))
        B, _, T = x.shape
        if T < MIN_FRAMES:
            raise ValueError("the Griffin-Lim decoder needs at least %d frames (reflect padding of 384 samples), got %d" % (MIN_FRAMES, T))
        if B < 1:
            raise ValueError("empty batch")
        n_iter = self.n_iter if n_iter is None else int(n_iter)
        momentum = self.momentum if momentum is None else float(momentum)
        if n_iter < 0 or not 0.0 <= momentum < 1.0:
            raise ValueError("n_iter must be >= 0 and momentum in [0, 1)")
        L = _hip.lib()
        with torch.no_grad(), torch.cuda.device(self.device):
            x = x.detach().to(torch.float32).contiguous()
            if kind == KIND_LINEAR and bool((x < 0).any()):
                raise ValueError("a magnitude must not be negative")
            if angles is None:
                ang = self.angles(B, T)
            elif isinstance(angles, str) and angles == ZERO_PHASE:
                ang = None
            else:
                if not isinstance(angles, torch.Tensor) or not angles.is_cuda or tuple(angles.shape) != (B, N_BIN, T, 2):
                    raise ValueError("angles: a HIP-device (re, im) tensor of shape %s" % ((B, N_BIN, T, 2),))
                ang = angles.detach().to(torch.float32).contiguous()
            n = L.mcvc_gl_workspace_floats(B, T)
            if n == 0:
                raise ValueError("batch of %d x %d frames is beyond the decoder's limits" % (B, T))
            ws = torch.empty(n, dtype=torch.float32, device=self.device)
            out = torch.empty(B, L.mcvc_gl_out_samples(T), dtype=torch.float32, device=self.device)
            _hip.check(L.mcvc_gl_decode(_hip.ptr(x), kind, _hip.ptr(ang), _hip.ptr(self.tables()), _hip.ptr(out), _hip.ptr(ws), n, B, T, n_iter,
                                        momentum, _hip.stream()), "mcvc_gl_decode")
        return out

    def inverse(self, mel, angles=None, n_iter=None, momentum=None):
        """[B, 80, T] log10-mel on the HIP device -> [B, 256 T] float32 waveform; one batched decode on the current stream."""
        if self._melinv is not None:
            return self.from_magnitude(self._melinv(mel), angles, n_iter, momentum)
        return self._decode(mel, KIND_LOGMEL, N_MEL, angles, n_iter, momentum)

    def from_magnitude(self, mag, angles=None, n_iter=None, momentum=None):
        """[B, 513, T] linear magnitude (>= 0) on the HIP device -> [B, 256 T] float32 waveform."""
        return self._decode(mag, KIND_LINEAR, N_BIN, angles, n_iter, momentum)

    def __call__(self, audio):
        from data_preprocessing.audio2mel import Audio2Mel
        if self._fft is None:
            self._fft = Audio2Mel(self.device)
        return self._fft(audio)
