"""float64 numpy restatement of the evaluation metric's definitions (mask_cyclegan_vc/metrics.py module docstring), written from them
and not from the kernel: the plain double loop over the cells, the same tie rule, a backtrack over stored choices.

    d(i, j)   = scale * sqrt(sum_k (x[k, i] - y[k, j])^2)
    acc(0, 0) = d(0, 0);  acc(i, j) = d(i, j) + min over the existing predecessors (i-1, j-1), (i-1, j), (i, j-1),
                taken in that order, replaced only on strict <;  len(i, j) = len(chosen predecessor) + 1, len(0, 0) = 1
    cepstra   c[k, t] = sum_m B[k, m] ln(10) mel[m, t], k = 1 .. n_cep, B the orthonormal DCT-II over 80 bins
"""
import math

import numpy as np

N_MEL = 80
MCD_SCALE = 10.0 / math.log(10.0) * math.sqrt(2.0)
STEPS = ((1, 1), (1, 0), (0, 1))                           # the predecessors (i - di, j - dj), in the order of the tie rule


def frame_distances(x, y, scale=1.0):
    """[K, Tx], [K, Ty] -> float64 [Tx, Ty]."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    diff = x[:, :, None] - y[:, None, :]
    return float(scale) * np.sqrt((diff * diff).sum(axis=0))


def dtw(x, y, scale=1.0, return_tables=False):
    """-> (cost, length, path int64 [length, 2]); with ``return_tables`` also (acc, len, choice)."""
    d = frame_distances(x, y, scale)
    Tx, Ty = d.shape
    acc = np.zeros((Tx, Ty))
    ln = np.zeros((Tx, Ty), dtype=np.int64)
    choice = np.full((Tx, Ty), -1, dtype=np.int64)
    for i in range(Tx):
        for j in range(Ty):
            if i == 0 and j == 0:
                acc[0, 0], ln[0, 0] = d[0, 0], 1
                continue
            best, which = None, -1
            for c, (di, dj) in enumerate(STEPS):
                pi, pj = i - di, j - dj
                if pi < 0 or pj < 0:
                    continue
                if best is None or acc[pi, pj] < best:
                    best, which = acc[pi, pj], c
            di, dj = STEPS[which]
            acc[i, j] = d[i, j] + best
            ln[i, j] = ln[i - di, j - dj] + 1
            choice[i, j] = which
    path = []
    i, j = Tx - 1, Ty - 1
    while True:
        path.append((i, j))
        if i == 0 and j == 0:
            break
        di, dj = STEPS[choice[i, j]]
        i, j = i - di, j - dj
    path = np.asarray(path[::-1], dtype=np.int64)
    out = (float(acc[-1, -1]), int(ln[-1, -1]), path)
    return out + (acc, ln, choice) if return_tables else out


def path_is_valid(path, Tx, Ty):
    path = np.asarray(path)
    if path.ndim != 2 or path.shape[1] != 2 or tuple(path[0]) != (0, 0) or tuple(path[-1]) != (Tx - 1, Ty - 1):
        return False
    steps = {tuple(s) for s in np.diff(path, axis=0).tolist()}
    return steps <= {(1, 1), (1, 0), (0, 1)}


def path_cost(x, y, path, scale=1.0):
    """Sum of the float64 frame distances along ``path``."""
    d = frame_distances(x, y, scale)
    path = np.asarray(path)
    return float(d[path[:, 0], path[:, 1]].sum())


def dct_basis(n_cep):
    """float64 [n_cep, 80]: rows 1 .. n_cep of the orthonormal DCT-II."""
    k = np.arange(1, n_cep + 1, dtype=np.float64)[:, None]
    m = np.arange(N_MEL, dtype=np.float64)[None, :]
    return math.sqrt(2.0 / N_MEL) * np.cos(math.pi * (2.0 * m + 1.0) * k / (2.0 * N_MEL))


def full_dct():
    """float64 [80, 80] including row 0 (1 / sqrt(80)): orthonormal."""
    B = np.empty((N_MEL, N_MEL))
    B[0] = 1.0 / math.sqrt(N_MEL)
    B[1:] = dct_basis(N_MEL - 1)
    return B


def mel_cepstra(mel, n_cep=24):
    """log10-mel [80, T] -> float64 [n_cep, T]."""
    return dct_basis(n_cep) @ (math.log(10.0) * np.asarray(mel, dtype=np.float64))


def mcd(converted_cep, target_cep):
    """cepstra [n_cep, T] of both sides -> (dB per frame of the path, path length)."""
    cost, length, _ = dtw(converted_cep, target_cep, MCD_SCALE)
    return cost / length, length
