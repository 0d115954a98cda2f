"""The pitch tracker's definition in float64 numpy (no project imports): YIN on the mel front-end's frame grid.

SR = 22050, hop 256, integration window W = 1024.  An utterance of L >= 385 samples has T = (L - 256) // 256 + 1 frames; frame t is centred
on sample c_t = 256 t + 128.  s = c_t - (W + tau_max) // 2, buf[j] = x[s + j] for 0 <= j < W + tau_max with zeros outside [0, L).

    d(tau)  = sum_{j < W} (buf[j] - buf[j + tau])^2                    (the direct difference form, tau = 0 .. tau_max)
    d'(0)   = 1,  d'(tau) = d(tau) tau / sum_{1 <= k <= tau} d(k),     1 where that sum is 0
    pick    : the first tau in tau_min .. tau_max with d'(tau) < thr, then upward while tau + 1 <= tau_max and d'(tau + 1) < d'(tau);
              a, b, c = d'(tau - 1), d'(tau), d'(tau + 1);  off = 0 at tau_max or where den = (a - b) + (c - b) <= 0, else
              clamp(0.5 (a - c) / den, -0.5, 0.5);  f0 = SR / (tau + off), aperiodicity = b
    unvoiced: no lag under thr -> f0 = 0, aperiodicity = min d' over tau_min .. tau_max
"""
import math

import numpy as np

SR = 22050
HOP = 256
W = 1024
MAX_LAG = 640


def lags(fmin=60.0, fmax=500.0):
    return int(math.ceil(SR / float(fmax))), int(math.floor(SR / float(fmin)))


def frames_of(n_samples):
    return (int(n_samples) - HOP) // HOP + 1


def frame_buffer(x, t, tau_max):
    """buf [W + tau_max] of frame t, float64, zeros outside the utterance."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    s = HOP * t + HOP // 2 - (W + tau_max) // 2
    n = W + tau_max
    buf = np.zeros(n, dtype=np.float64)
    lo, hi = max(s, 0), min(s + n, x.size)
    if hi > lo:
        buf[lo - s:hi - s] = x[lo:hi]
    return buf


def difference(x, t, tau_max):
    """d [tau_max + 1] of frame t."""
    buf = frame_buffer(x, t, tau_max)
    win = np.lib.stride_tricks.sliding_window_view(buf, W)[:tau_max + 1]          # row tau = buf[tau : tau + W]
    diff = win - buf[None, :W]
    return np.einsum("ij,ij->i", diff, diff)


def cmnd(d):
    """d' [tau_max + 1] from d."""
    d = np.asarray(d, dtype=np.float64)
    out = np.ones_like(d)
    cs = np.cumsum(d[1:])
    tau = np.arange(1, d.size, dtype=np.float64)
    ok = cs > 0
    out[1:][ok] = d[1:][ok] * tau[ok] / cs[ok]
    return out


def _walk(dp, tau_min, tau_max, thr):
    """-> (tau or 0, [(lhs, rhs) of every comparison made])."""
    cmp = []
    for tau in range(tau_min, tau_max + 1):
        cmp.append((float(dp[tau]), float(thr)))
        if dp[tau] < thr:
            while tau + 1 <= tau_max:
                cmp.append((float(dp[tau + 1]), float(dp[tau])))
                if not dp[tau + 1] < dp[tau]:
                    break
                tau += 1
            return tau, cmp
    return 0, cmp


def pick(dp, tau_min, tau_max, thr):
    """-> (voiced, tau, off, f0, aperiodicity); tau = 0 and off = 0 when unvoiced."""
    dp = np.asarray(dp, dtype=np.float64)
    tau, _ = _walk(dp, tau_min, tau_max, thr)
    if tau == 0:
        return False, 0, 0.0, 0.0, float(dp[tau_min:tau_max + 1].min())
    a, b = float(dp[tau - 1]), float(dp[tau])
    off = 0.0
    if tau < tau_max:
        c = float(dp[tau + 1])
        den = (a - b) + (c - b)
        if den > 0:
            off = min(max(0.5 * (a - c) / den, -0.5), 0.5)
    return True, tau, off, SR / (tau + off), b


def comparisons(dp, tau_min, tau_max, thr):
    """Every (lhs, rhs) pair the pick rule compared with `<`: d'(tau) against thr while scanning, d'(tau + 1) against d'(tau) while descending."""
    return _walk(np.asarray(dp, dtype=np.float64), tau_min, tau_max, thr)[1]


def track(x, tau_min=45, tau_max=367, thr=0.15):
    """-> f0 [T], aperiodicity [T], d' [tau_max + 1, T], tau [T] (0 = unvoiced), all from float64 arithmetic on the samples as given."""
    x = np.asarray(x).reshape(-1)
    T = frames_of(x.size)
    f0, ap, taus = np.zeros(T), np.zeros(T), np.zeros(T, dtype=np.int64)
    dps = np.ones((tau_max + 1, T))
    for t in range(T):
        dp = cmnd(difference(x, t, tau_max))
        dps[:, t] = dp
        _, taus[t], _, f0[t], ap[t] = pick(dp, tau_min, tau_max, thr)
    return f0, ap, dps, taus
