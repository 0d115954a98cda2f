"""Float64 closed form of the sample-rate conversion (include/mcvc.h, "sample-rate conversion"), written from the definition and not from the
product code: the direct sum over input samples, no polyphase split.

    m = max(up, down), half = 10 m
    h[n] = up * w[n] / sum(w),  w[n] = (1/m) sinc((n - half) / m) * kaiser(2 half + 1, 5.0)[n],  n = 0 .. 2 half
    n_out = ceil(n_in up / down)
    y[k] = sum_i x[i] h[k down + half - i up]   over 0 <= i < n_in with 0 <= k down + half - i up <= 2 half

tests/test_host_resample.py pins this to scipy.signal.resample_poly at 1e-12, so the GPU tests need scipy's conventions nowhere else.
"""
import numpy as np

U = 2.0 ** -24                     # unit roundoff of float32


def taps(up, down):
    m = max(up, down)
    half = 10 * m
    n = np.arange(2 * half + 1, dtype=np.float64)
    w = np.sinc((n - half) / m) / m * np.kaiser(2 * half + 1, 5.0)
    return up * (w / np.sum(w))


def out_len(n_in, up, down):
    return (n_in * up + down - 1) // down


def resample(x, up, down, h=None):
    """-> (y, mag, terms): y float64 [n_out]; mag[k] = sum_i |x[i]| |h[..]| and terms[k] = the number of terms of output k."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    h = taps(up, down) if h is None else np.asarray(h, dtype=np.float64)
    half = 10 * max(up, down)
    assert h.size == 2 * half + 1
    n_in = x.size
    n_out = out_len(n_in, up, down)
    y, mag, terms = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out, dtype=np.int64)
    width = 2 * half // up + 2                                            # no output has more candidate inputs than this
    for k0 in range(0, n_out, 4096):
        k = np.arange(k0, min(n_out, k0 + 4096), dtype=np.int64)
        c = k * down + half
        i = (c // up)[:, None] - np.arange(width, dtype=np.int64)[None, :]       # the largest i with a non-negative tap index, downwards
        t = c[:, None] - i * up
        ok = (i >= 0) & (i < n_in) & (t >= 0) & (t <= 2 * half)
        xv = np.where(ok, x[np.clip(i, 0, n_in - 1)], 0.0)
        hv = np.where(ok, h[np.clip(t, 0, 2 * half)], 0.0)
        y[k] = np.sum(xv * hv, axis=1)
        mag[k] = np.sum(np.abs(xv) * np.abs(hv), axis=1)
        terms[k] = ok.sum(axis=1)
    return y, mag, terms


def gate(mag, terms):
    """Per output: 1.01 (n_k + 2) 2^-24 sum |x_i| |h_j| -- one rounding per tap and per product, n_k for the sums; any order, FMA or not."""
    return 1.01 * (terms + 2) * U * mag


def check(name, got, x32, up, down):
    """got (float32, from the device) against the checker fed the same float32 input and the float64 taps; -> the largest error / gate."""
    got = np.asarray(got)
    ref, mag, terms = resample(np.asarray(x32, dtype=np.float32), up, down)
    assert got.dtype == np.float32 and got.shape == ref.shape, (name, got.dtype, got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    g = gate(mag, terms)
    worst = float(np.max(np.where(err > 0, err / np.maximum(g, 1e-300), 0.0))) if err.size else 0.0
    print("%s: %d -> %d samples at %d/%d  max err %.3e  worst err / gate %.3f" % (name, np.asarray(x32).size, got.size, up, down, float(err.max()), worst))
    assert (err <= g).all(), (name, worst)
    return worst
