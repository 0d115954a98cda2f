"""Checker of the mel inversion (mask_cyclegan_vc/melinv.py, csrc/melinv_kernels.hip), shared by test_host_melinv.py,
test_hip_melinv.py and tools/melinv_bench.py: the definition in numpy with dense products.  Nothing here comes from the code under test.

    B   audio_checker.slaney_mel_basis(), float64 [80, 513];  P = numpy.linalg.pinv(B);  lambda = numpy.linalg.norm(B, 2) ** 2
    s = 1 / lambda;  beta_k = (t_k - 1) / t_k+1,  t_0 = 1,  t_k+1 = (1 + sqrt(1 + 4 t_k ** 2)) / 2
    B, P, s and beta_k are computed in float64 and USED AS FLOAT32 -- in both precisions below: the rounded tables are the definition
    y = 10 ** logmel;  M_0 = max(0, P y);  Z_0 = M_0
    k < n_iter:  r = B Z_k - y;  M_k+1 = max(0, Z_k - s B^T r);  Z_k+1 = M_k+1 + beta_k (M_k+1 - M_k);  result M_n_iter

``solve(logmel, n_iter, numpy.float64)`` is the truth, ``solve(..., numpy.float32)`` the yardstick: float32 storage and float32 dense
products (numpy's own summation order, not the kernel's).  The problem is underdetermined, so rounding drifts along the null space of B
and the float32 distance grows with n_iter; a gate follows that distance, not a constant.
"""
import numpy as np

import audio_checker as ack

N_MEL, N_BIN = ack.N_MEL, ack.N_FFT // 2 + 1
MAX_ITER = 512
FLOOR = 2e-6                                                # the project's floor for unit-scale signals, times the frame's largest magnitude
CHAIN_FACTOR = 4                                            # the project's factor for long chains

_B64 = ack.slaney_mel_basis()
_P64 = np.linalg.pinv(_B64)
_LAMBDA = float(np.linalg.norm(_B64, 2) ** 2)


def basis():
    return _B64.copy()


def pinv_basis():
    return _P64.copy()


def lipschitz():
    return _LAMBDA


def betas(n):
    """float64 [n]."""
    out, t = np.empty(n), 1.0
    for k in range(n):
        tn = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        out[k] = (t - 1.0) / tn
        t = tn
    return out


def _tables(dtype):
    """The float32-rounded constants, held in ``dtype``."""
    f = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(dtype)
    return f(_B64), f(_P64), f(1.0 / _LAMBDA), f(betas(MAX_ITER))


def _frames(logmel, dtype):
    x = np.asarray(logmel)
    assert x.ndim == 3 and x.shape[1] == N_MEL, x.shape
    return np.ascontiguousarray(np.moveaxis(x, 1, 0).reshape(N_MEL, -1)).astype(dtype), x.shape[0], x.shape[2]


def _unframe(M, Bn, T):
    return np.ascontiguousarray(np.moveaxis(M.reshape(N_BIN, Bn, T), 0, 1))


def start(logmel, dtype=np.float64):
    """[B, 80, T] -> max(0, P 10 ** logmel) [B, 513, T] in ``dtype`` arithmetic."""
    x, Bn, T = _frames(logmel, dtype)
    _, P, _, _ = _tables(dtype)
    return _unframe(np.maximum(P @ np.power(dtype(10.0), x), dtype(0.0)), Bn, T)


def solve(logmel, n_iter, dtype=np.float64):
    """[B, 80, T] log10-mel -> M_n_iter [B, 513, T] in ``dtype`` arithmetic (dense products)."""
    assert 0 <= n_iter <= MAX_ITER
    x, Bn, T = _frames(logmel, dtype)
    Bm, P, s, beta = _tables(dtype)
    y = np.power(dtype(10.0), x)
    M = np.maximum(P @ y, dtype(0.0))
    Z = M.copy()
    for k in range(n_iter):
        r = Bm @ Z - y
        Mn = np.maximum(Z - s * (Bm.T @ r), dtype(0.0))
        Z = Mn + beta[k] * (Mn - M)
        M = Mn
        assert M.dtype == dtype and Z.dtype == dtype
    return _unframe(M, Bn, T)


def mel_residual(M, logmel):
    """|| B M - y || / || y || over the whole tensor, float64 with the float64 basis."""
    M = np.asarray(M, dtype=np.float64)
    y = np.power(10.0, np.asarray(logmel, dtype=np.float64))
    return float(np.linalg.norm(np.einsum("jb,nbt->njt", _B64, M) - y) / np.linalg.norm(y))


def relative_distance(M, S):
    """|| M - S || / || S ||, float64."""
    M, S = np.asarray(M, dtype=np.float64), np.asarray(S, dtype=np.float64)
    return float(np.linalg.norm(M - S) / np.linalg.norm(S))


def frame_gate(got, truth, ref32):
    """Per frame [B, T]: (the largest distance of ``got`` from the truth, the gate
    max(FLOOR x the frame's largest float64 magnitude, CHAIN_FACTOR x the float32 checker's largest distance in that frame))."""
    got, truth, ref32 = (np.asarray(a, dtype=np.float64) for a in (got, truth, ref32))
    d = np.abs(got - truth).max(axis=1)
    gate = np.maximum(FLOOR * np.abs(truth).max(axis=1), CHAIN_FACTOR * np.abs(ref32 - truth).max(axis=1))
    return d, gate
