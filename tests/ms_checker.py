"""float64 numpy restatement of the modulation-spectrum definitions (mask_cyclegan_vc/metrics.py module docstring), written from them and
not from the kernel: numpy's FFT of the zero-padded, mean-removed trajectory.

    mean[k]  = (1/T) sum_t c[k, t];  x[t] = c[k, t] - mean[k];  var[k] = (1/T) sum_t x[t]^2
    X[f]     = sum_{t < T} x[t] exp(-2 pi i f t / n_fft), f = 1 .. n_fft / 2;  P[k, f] = |X[f]|^2 / T;  bin f at f (22050 / 256) / n_fft Hz
    LMS[k,f] = (1/n) sum_u 10 log10(max(P[u, k, f], floor));  LGV[k] = (1/n) sum_u 10 log10(max(var[u, k], floor));  floor = 1e-10
    msd_per_dim[k] = sqrt((1/F) sum_f (LMS_A - LMS_B)^2);  msd = sqrt((1/(K F)) sum_{k, f} (..)^2);  gvd = sqrt((1/K) sum_k (LGV_A - LGV_B)^2)

The mean and the variance are taken from float64 copies of the (float32) input.
"""
import numpy as np

FLOOR = 1e-10
FRAME_RATE = 22050.0 / 256.0
FFTS = (1024, 2048, 4096)


def spectrum(c, n_fft):
    """[K, T] -> (X complex128 [K, n_fft / 2] (bins 1 .. n_fft / 2), x float64 [K, T], mean [K], var [K])."""
    c = np.asarray(c, dtype=np.float64)
    K, T = c.shape
    assert n_fft in FFTS and 1 <= T <= n_fft
    mean = c.sum(axis=1) / T
    x = c - mean[:, None]
    var = (x * x).sum(axis=1) / T
    X = np.fft.rfft(x, n_fft, axis=1)[:, 1:]
    return X, x, mean, var


def power(c, n_fft):
    """[K, T] -> (P [K, n_fft / 2], mean [K], var [K])."""
    X, _, mean, var = spectrum(c, n_fft)
    return (X.real ** 2 + X.imag ** 2) / np.asarray(c).shape[1], mean, var


def mean_log(values, floor=FLOOR):
    """[n, ...] -> [...] in dB."""
    v = np.asarray(values, dtype=np.float64)
    return (10.0 * np.log10(np.maximum(v, floor))).sum(axis=0) / v.shape[0]


def bin_hz(n_fft):
    return np.arange(1, n_fft // 2 + 1) * FRAME_RATE / n_fft


def bins_used(n_fft, max_hz=None):
    if max_hz is None:
        return n_fft // 2
    return int(np.count_nonzero(bin_hz(n_fft) <= max_hz * (1.0 + 1e-12)))


def distance(a, b, n_used=None):
    """tables [K, n_bins] -> (per_dim [K], total)."""
    a, b = np.atleast_2d(np.asarray(a, dtype=np.float64)), np.atleast_2d(np.asarray(b, dtype=np.float64))
    F = a.shape[1] if n_used is None else n_used
    d2 = (a[:, :F] - b[:, :F]) ** 2
    return np.sqrt(d2.sum(axis=1) / F), float(np.sqrt(d2.sum() / (a.shape[0] * F)))


def tables(ceps, n_fft):
    """list of [K, T_i] -> (LMS [K, n_fft / 2], LGV [K])."""
    res = [power(c, n_fft) for c in ceps]
    return mean_log(np.stack([r[0] for r in res])), mean_log(np.stack([r[2] for r in res]))


def msd(ceps_a, ceps_b, n_fft=4096, max_hz=None):
    """Two lists of cepstra [K, T_i] -> dict msd, msd_per_dim, gvd, lms_a, lms_b, lgv_a, lgv_b, n_bins_used."""
    lms_a, lgv_a = tables(ceps_a, n_fft)
    lms_b, lgv_b = tables(ceps_b, n_fft)
    F = bins_used(n_fft, max_hz)
    per_dim, total = distance(lms_a, lms_b, F)
    return {"msd": total, "msd_per_dim": per_dim, "gvd": distance(lgv_a[None, :], lgv_b[None, :])[1], "lms_a": lms_a, "lms_b": lms_b,
            "lgv_a": lgv_a, "lgv_b": lgv_b, "n_bins_used": F}


def trajectory(rs, K, T, noise=0.05):
    """The tests' cepstra: a random walk plus white noise, 0.1 cumsum(N(0, 1)) + noise N(0, 1), float32 [K, T]."""
    return (0.1 * np.cumsum(rs.randn(K, T), axis=1) + noise * rs.randn(K, T)).astype(np.float32)
