"""Mel inversion by non-negative least squares on the HIP kernel (csrc/melinv_kernels.hip through ``mcvc_melinv_solve``): the
magnitude the Griffin-Lim decoder starts from, made consistent with the mel-spectrogram that was asked for.

``max(0, pinv(B) @ 10**logmel)`` -- the decoder's default -- is a magnitude whose own mel-spectrogram is not the input any more.
``MelInverter`` solves ``min_{M >= 0} || B M - y ||``, ``y = 10**logmel``, per frame, by a FIXED number of accelerated projected-gradient
(FISTA) steps from that very start value.  80 equations, 513 unknowns: the minimiser is not unique, so the result is defined by the
iteration, not by "the NNLS solution" (an active-set solver reaches the same residual with at most 80 spikes per frame):

    B    float64 [80, 513] Slaney basis (data_preprocessing.audio2mel.mel_filterbank), used as float32
    P    float64 pinv(B), used as float32 -- the table the decoder uploads
    s    1 / lambda, lambda = numpy.linalg.norm(B, 2) ** 2 (1.128e-3), float64, used as float32
    beta_k = (t_k - 1) / t_k+1,  t_0 = 1,  t_k+1 = (1 + sqrt(1 + 4 t_k ** 2)) / 2, float64, used as float32

    M_0 = max(0, P y)   (exp10f and one fmaf chain over the 80 filters: bit for bit the decoder's start value),  Z_0 = M_0
    k < n_iter:  r = B Z_k - y;  M_k+1 = max(0, Z_k - s B^T r);  Z_k+1 = M_k+1 + beta_k (M_k+1 - M_k)
    result M_n_iter;  no restart, no stopping test;  0 <= n_iter <= 512, default 64

* ``inv = MelInverter(device=None, n_iter=64)``
* ``inv(logmel)`` / ``inv.inv(logmel, n_iter=None)``  [B, 80, T] log10-mel on the HIP device -> [B, 513, T] float32, one launch on the
  current stream, no autograd.  ``GriffinLimVocoder(mel_inverse="nnls")`` feeds it to ``from_magnitude``.

Every sum has one order and nothing is shared between frames, so a frame's result does not depend on its batch, its position or T.
Not verified against librosa: it does not exist here; librosa solves the same problem with L-BFGS-B, so samples differ.  The checker is
the float64 restatement tests/melinv_checker.py.  There is no CPU path.
"""
import numpy as np
import torch

from . import _hip

N_MEL = 80
N_BIN = 513
DEFAULT_ITER = 64
MAX_ITER = 512                       # mcvc_melinv_max_iter()


def lipschitz():
    """float64: the largest eigenvalue of B B^T, the Lipschitz constant of the gradient of 0.5 || B M - y ||^2."""
    from data_preprocessing.audio2mel import mel_filterbank
    return float(np.linalg.norm(mel_filterbank(np.float64), 2) ** 2)


def host_tables(basis=None, pinv=None, lam=None):
    """The solver's constant operand as a float32 host array (``mcvc_melinv_tables_init``); raises where the library refuses the basis."""
    from data_preprocessing.audio2mel import mel_filterbank
    from .griffinlim import pinv_mel_basis
    L = _hip.lib()
    basis = np.ascontiguousarray(mel_filterbank(np.float64) if basis is None else basis, dtype=np.float32)
    pinv = np.ascontiguousarray(pinv_mel_basis() if pinv is None else pinv, dtype=np.float32)
    if basis.shape != (N_MEL, N_BIN) or pinv.shape != (N_BIN, N_MEL):
        raise ValueError("basis [80, 513] and pinv [513, 80], got %s and %s" % (basis.shape, pinv.shape))
    host = np.zeros(L.mcvc_melinv_tables_floats(), dtype=np.float32)
    _hip.check(L.mcvc_melinv_tables_init(basis.ctypes.data, pinv.ctypes.data, lipschitz() if lam is None else float(lam), host.ctypes.data),
               "mcvc_melinv_tables_init (a column of the basis with more than two non-zeros, or non-adjacent ones?)")
    return host


def check_n_iter(n_iter, what="n_iter"):
    n = int(n_iter)
    if not 0 <= n <= MAX_ITER:
        raise ValueError("%s must lie in [0, %d], got %r" % (what, MAX_ITER, n_iter))
    return n


class MelInverter(object):
    """``MelInverter(device=None, n_iter=64)``; then ``inv(logmel, n_iter=None)`` or the call itself."""

    def __init__(self, device=None, n_iter=DEFAULT_ITER):
        self.device = _hip.hip_device("mask_cyclegan_vc.melinv", device)
        self.n_iter = check_n_iter(n_iter)

    def tables(self):
        return _hip.device_constant("melinv.tables", self.device, host_tables)

    def inv(self, logmel, n_iter=None):
        """[B, 80, T] log10-mel on the HIP device -> [B, 513, T] float32 magnitude, T >= 1."""
        _hip.require_on_device("mask_cyclegan_vc.melinv", logmel, self.device, "input", "solver")
        if logmel.dim() != 3 or logmel.shape[1] != N_MEL:
            raise ValueError("expected a [B, %d, T] tensor, got %s" % (N_MEL, tuple(logmel.shape)))
        B, _, T = logmel.shape
        if B < 1 or T < 1:
            raise ValueError("empty batch")
        n_iter = self.n_iter if n_iter is None else check_n_iter(n_iter)
        L = _hip.lib()
        with torch.no_grad(), torch.cuda.device(self.device):
            x = logmel.detach().to(torch.float32).contiguous()
            out = torch.empty(B, N_BIN, T, dtype=torch.float32, device=self.device)
            rc = L.mcvc_melinv_solve(_hip.ptr(x), _hip.ptr(self.tables()), _hip.ptr(out), B, T, n_iter, _hip.stream())
            if rc == 1001:
                raise ValueError("batch of %d x %d frames is beyond the solver's limits" % (B, T))
            _hip.check(rc, "mcvc_melinv_solve")
        return out

    __call__ = inv
