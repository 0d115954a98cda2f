"""Objective evaluation on the HIP kernels: batched dynamic time warping and mel-cepstral distortion (csrc/dtw_kernels.hip through
``mcvc_cep_project`` and ``mcvc_dtw_run``).  All arithmetic runs in the kernels; Python builds tables and moves data.  There is no CPU path.

* ``dtw(x, y, scale=1.0, return_path=False)``   ragged batch of pairs -> cost [n], length [n] (and the warping paths);
* ``mel_cepstra(mels, n_cep=24)``               log10-mels [80, T_i] -> cepstra bank ([n_cep, N], offsets);
* ``mcd(converted_mels, target_mels, n_cep=24)`` -> per-pair dB, path lengths and the mean;
* ``f0_stats(f0_x, f0_y, paths)``                F0 tracks + warping paths -> per-pair F0 RMSE / bias in cents and voiced/unvoiced error;
* ``f0_distortion(conv_wavs, tgt_wavs, conv_mels, tgt_mels, n_cep=24, tracker=None)`` -> the same from waveforms and their log-mels;
* ``modulation_spectrum(feats, n_fft=4096)``     ragged batch -> modulation power [n, K, n_fft/2], mean and global variance [n, K];
* ``msd(converted_mels, target_mels, n_cep=24, n_fft=4096, max_hz=None)`` -> modulation-spectrum distance and GV distance of two SETS.

Definitions (tests/dtw_checker.py restates them in float64):

Features.  A bank is [K, N] float32, time-contiguous per row: utterances concatenated along time, with frame offsets offs[n + 1];
1 <= K <= 80.  ``x`` / ``y`` are lists of [K, T_i] tensors or arrays, or ``(bank, offs)`` pairs already on the device.

Cepstra from the project's log10-mels [80, T]:  c[k, t] = sum_m B[k, m] * ln(10) * mel[m, t] for k = 1 .. n_cep, B the orthonormal DCT-II
over the 80 mel bins (B[k, m] = sqrt(2 / 80) cos(pi (m + 1/2) k / 80)); c_0, the energy term, is dropped.  The basis is computed in float64
on the host, rounded once and uploaded once per device.

Frame distance.  d(i, j) = scale * sqrt(sum_k (x[k, i] - y[k, j])^2), computed from differences.  For MCD, scale = (10 / ln 10) sqrt(2): dB.

DTW.  acc(0, 0) = d(0, 0); acc(i, j) = d(i, j) + min over the existing predecessors (i-1, j-1), (i-1, j), (i, j-1), taken in that order
and replaced only on strict <; len(i, j) = len(chosen predecessor) + 1 with len(0, 0) = 1.  Per pair cost = acc(Tx-1, Ty-1) and
length = len(Tx-1, Ty-1); on request the path as int32 [length, 2] from (0, 0) to (Tx-1, Ty-1).  MCD = cost / length: the mean over the
warping path that espnet-style evaluation scripts report.

Comparability.  These cepstra come from an 80-band mel spectrum, NOT from WORLD mel-cepstral coefficients: the numbers compare runs of this
project with one another (checkpoints, ``--dtype`` settings, decoders), not with the tables of papers.

A batch equals its single calls bit for bit: every pair is one wavefront that sees only its own two utterances.  The default call writes
no Tx x Ty matrix; ``return_path=True`` stores one direction byte per cell and a second launch walks them back.

F0 statistics (csrc/f0_kernels.hip through ``mcvc_f0_stats``; the tracks come from mask_cyclegan_vc/pitch.py, 0 = unvoiced).  Over the rows
(i, j) of a pair's warping path: counts of rows with both sides voiced, x only, y only, neither; over the both-voiced rows
c = 1200 log2(fx[i] / fy[j]) cents, ``bias_cents`` = mean c, ``rmse_cents`` = sqrt(mean c^2), ``vuv_error`` = (x only + y only) / length.
A pair without a both-voiced row has ``voiced_pairs`` 0 and ``nan`` for the two cent figures: a documented value, not an exception.
One wavefront per pair, a fixed reduction order, no atomics: a batch equals its single calls bit for bit.

Modulation spectra and global variance (csrc/ms_kernels.hip through ``mcvc_ms_power``, ``mcvc_ms_mean_log`` and ``mcvc_ms_distance``;
tests/ms_checker.py restates this in float64).  These need no alignment and no parallel sentences: they compare two *sets* of utterances.
Input: a cepstra bank [K, N] with offsets as ``mel_cepstra`` returns it, 1 <= K <= 80; utterance u has T frames; ``n_fft`` is 1024, 2048 or
4096 (the default, = ``max_frames()``), and T <= n_fft: a longer utterance is refused, nothing is truncated.  Per utterance and row k:
mean[u, k] = (1/T) sum_t c[k, t];  x[t] = c[k, t] - mean[u, k];  var[u, k] = (1/T) sum_t x[t]^2, the population variance from the deviations
(never E[c^2] - E[c]^2);  X[f] = sum_{t < T} x[t] exp(-2 pi i f t / n_fft) for f = 1 .. n_fft / 2: a rectangular window zero-padded to
n_fft, bin 0 dropped because the mean was removed;  modulation power P[u, k, f] = |X[f]|^2 / T;  bin f lies at f (22050 / 256) / n_fft Hz.
Twiddles come from a table of cos(2 pi j / n_fft), j < n_fft, computed in float64 on the host, rounded once and uploaded once per device
and n_fft; the sine is the same table a quarter turn on; the table is indexed with the *integer* phase (f t) mod n_fft -- exact argument
reduction, the phase is never formed in floating point.  Per set of n utterances, with floor = 1e-10 (a definition, not a tolerance):
LMS[k, f] = (1/n) sum_u 10 log10(max(P[u, k, f], floor)) and LGV[k] = (1/n) sum_u 10 log10(max(var[u, k], floor)), in dB, utterances
summed in index order.  Between two sets A and B, which may differ in size and need not be parallel, over the F bins at or below
``max_hz`` (default: all n_fft / 2 bins, up to Nyquist = 43.07 Hz):  msd_per_dim[k] = sqrt((1/F) sum_f (LMS_A - LMS_B)^2),
msd = sqrt((1/(K F)) sum_{k, f} (LMS_A - LMS_B)^2),  gvd = sqrt((1/K) sum_k (LGV_A - LGV_B)^2), all in dB.  No atomics, every reduction in a
fixed order; an utterance's P, mean and var depend on that utterance alone, so a ragged batch equals its single calls bit for bit.  One
``msd()`` is 2 + 4 + 2 = ``mcvc_ms_launches()`` = 8 launches after the two cepstra projections.  Comparability: as for MCD the cepstra
come from the 80-band log-mel, not from WORLD, at 86.13 frames per second, not 200: the numbers compare runs of this project.
"""
import ctypes
import math

import numpy as np
import torch

from . import _hip

N_MEL = 80
MAX_K = 80
TABLE_COLS = 6
MCD_SCALE = (10.0 / math.log(10.0)) * math.sqrt(2.0)
MS_FFTS = (1024, 2048, 4096)
MS_FLOOR = 1e-10
FRAME_RATE = 22050.0 / 256.0


def dct_basis(n_cep):
    """float64 [n_cep, 80]: rows 1 .. n_cep of the orthonormal DCT-II over the 80 mel bins."""
    n_cep = int(n_cep)
    if not 1 <= n_cep <= N_MEL - 1:
        raise ValueError("n_cep must lie in 1 .. %d, got %r" % (N_MEL - 1, n_cep))
    k = np.arange(1, n_cep + 1, dtype=np.float64)[:, None]
    m = np.arange(N_MEL, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / N_MEL) * np.cos(np.pi * (m + 0.5) * k / N_MEL)


def host_basis(n_cep):
    """The projection's constant operand as a float32 host array (``mcvc_cep_basis_init``)."""
    n_cep = int(n_cep)
    if not 1 <= n_cep <= N_MEL - 1:
        raise ValueError("n_cep must lie in 1 .. %d, got %r" % (N_MEL - 1, n_cep))
    host = np.empty((n_cep, N_MEL), dtype=np.float32)
    _hip.check(_hip.lib().mcvc_cep_basis_init(n_cep, host.ctypes.data), "mcvc_cep_basis_init")
    return host


def max_frames():
    return int(_hip.lib().mcvc_dtw_max_frames())


def bank(feats, device=None, rows=None):
    """list of [K, T_i] (tensors or arrays) or ``(bank, offs)`` -> (float32 device tensor [K, N], int32 numpy offsets [n + 1]).
    Shapes, finiteness and the device are checked here."""
    dev = _hip.hip_device("mask_cyclegan_vc.metrics", device)
    if isinstance(feats, tuple) and len(feats) == 2 and isinstance(feats[0], torch.Tensor) and feats[0].dim() == 2 and not isinstance(feats[1], torch.Tensor):
        b, offs = feats
        _hip.require_on_device("mask_cyclegan_vc.metrics", b, dev, "bank", "metrics")
        offs = np.ascontiguousarray(offs, dtype=np.int64).reshape(-1)
        if offs.size < 2 or offs[0] != 0 or offs[-1] != b.shape[1] or bool((np.diff(offs) < 1).any()):
            raise ValueError("offsets must rise from 0 to the bank's %d frames" % b.shape[1])
        b = b.detach().to(torch.float32).contiguous()
    else:
        items = list(feats)
        if not items:
            raise ValueError("empty batch")
        ts = []
        for f in items:
            t = f.detach() if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f))
            if t.dim() != 2 or t.shape[1] < 1 or t.shape[0] != items[0].shape[0]:
                raise ValueError("expected [K, T] features with one K and T >= 1, got %s" % (tuple(t.shape),))
            ts.append(t.to(dev, torch.float32))
        offs = np.zeros(len(ts) + 1, dtype=np.int64)
        np.cumsum([t.shape[1] for t in ts], out=offs[1:])
        b = torch.cat(ts, dim=1).contiguous() if len(ts) > 1 else ts[0].contiguous()
    if rows is not None and b.shape[0] != rows:
        raise ValueError("expected [%d, T] features, got %d rows" % (rows, b.shape[0]))
    if not 1 <= b.shape[0] <= MAX_K:
        raise ValueError("features have between 1 and %d rows, got %d" % (MAX_K, b.shape[0]))
    if offs[-1] >= 2 ** 31:
        raise ValueError("a bank holds at most 2^31 - 1 frames")
    if not bool(torch.isfinite(b).all()):
        raise ValueError("features must be finite")
    return b, offs.astype(np.int32)


def split(b, offs):
    """(bank, offs) -> list of [K, T_i] views."""
    return [b[:, int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


def plan(x_offs, y_offs, want_path):
    """HOST tables -> (table int64 [n, 6], workspace bytes, path rows) through ``mcvc_dtw_plan``; raises on what it refuses."""
    L = _hip.lib()
    x_offs = np.ascontiguousarray(x_offs, dtype=np.int32)
    y_offs = np.ascontiguousarray(y_offs, dtype=np.int32)
    n = x_offs.size - 1
    if n < 1 or y_offs.size != x_offs.size:
        raise ValueError("x and y must hold the same number (>= 1) of utterances, got %d and %d" % (x_offs.size - 1, y_offs.size - 1))
    table = np.zeros((n, TABLE_COLS), dtype=np.int64)
    ws, rows = ctypes.c_longlong(0), ctypes.c_longlong(0)
    rc = L.mcvc_dtw_plan(x_offs.ctypes.data, y_offs.ctypes.data, n, int(bool(want_path)), table.ctypes.data, ctypes.byref(ws), ctypes.byref(rows))
    if rc != 0:
        raise ValueError("mcvc_dtw_plan refused the batch (code %d): every utterance needs between 1 and %d frames" % (rc, L.mcvc_dtw_max_frames()))
    return table, int(ws.value), int(rows.value)


def dtw(x, y, scale=1.0, return_path=False):
    """Ragged batch of pairs (utterance p of ``x`` against utterance p of ``y``) in one launch (two with paths), on the current stream.
    -> (cost float32 [n], length int32 [n]) device tensors, and with ``return_path`` a list of int32 [length_p, 2] device tensors."""
    xb, xo = bank(x)
    yb, yo = bank(y, xb.device)
    if xb.shape[0] != yb.shape[0]:
        raise ValueError("x has %d feature rows, y has %d" % (xb.shape[0], yb.shape[0]))
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError("scale must be finite, got %r" % (scale,))
    table, ws_bytes, rows = plan(xo, yo, return_path)
    n = table.shape[0]
    L = _hip.lib()
    dev = xb.device
    with torch.no_grad(), torch.cuda.device(dev):
        table_d = torch.from_numpy(table).to(dev)
        cost = torch.empty(n, dtype=torch.float32, device=dev)
        length = torch.empty(n, dtype=torch.int32, device=dev)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        path = torch.empty(max(rows, 1), 2, dtype=torch.int32, device=dev) if return_path else None
        _hip.check(L.mcvc_dtw_run(_hip.ptr(xb), xb.shape[1], _hip.ptr(yb), yb.shape[1], xb.shape[0], scale, xo.ctypes.data, yo.ctypes.data,
                                  _hip.ptr(table_d), n, _hip.ptr(cost), _hip.ptr(length), _hip.ptr(path), _hip.ptr(ws), ws_bytes, _hip.stream()),
                   "mcvc_dtw_run")
        if not return_path:
            return cost, length
        lens = length.cpu().numpy()
        paths = [path[int(table[p, 5]):int(table[p, 5]) + int(lens[p])] for p in range(n)]
    return cost, length, paths


def mel_cepstra(mels, n_cep=24):
    """log10-mels (list of [80, T_i], or a bank) -> (cepstra bank float32 [n_cep, N] on the device, int32 offsets); one launch."""
    b, offs = bank(mels, rows=N_MEL)
    n_cep = int(n_cep)
    if not 1 <= n_cep <= N_MEL - 1:
        raise ValueError("n_cep must lie in 1 .. %d, got %r" % (N_MEL - 1, n_cep))
    dev = b.device
    basis = _hip.device_constant(("metrics.dct_basis", n_cep), dev, lambda: host_basis(n_cep))
    with torch.no_grad(), torch.cuda.device(dev):
        out = torch.empty(n_cep, b.shape[1], dtype=torch.float32, device=dev)
        _hip.check(_hip.lib().mcvc_cep_project(_hip.ptr(b), b.shape[1], _hip.ptr(basis), n_cep, _hip.ptr(out), _hip.stream()), "mcvc_cep_project")
    return out, offs


def mcd(converted_mels, target_mels, n_cep=24):
    """Mel-cepstral distortion after DTW alignment, pair by pair -> dict: ``mcd`` (dB per pair, float64 numpy: float32 cost / length),
    ``length`` (path lengths), ``frames_converted`` / ``frames_target``, ``mean``."""
    cx, xo = mel_cepstra(converted_mels, n_cep)
    cy, yo = mel_cepstra(target_mels, n_cep)
    cost, length = dtw((cx, xo), (cy, yo), scale=MCD_SCALE)
    cost, length = cost.cpu().numpy().astype(np.float64), length.cpu().numpy()
    per = cost / length
    return {"mcd": per, "length": length, "frames_converted": np.diff(xo), "frames_target": np.diff(yo), "mean": float(per.mean()), "n_cep": int(n_cep)}


def _tracks(tracks, dev):
    """list of 1-D F0 tracks -> (float32 device bank [N], int64 offsets [n + 1])."""
    ts = []
    for f in tracks:
        t = f.detach() if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f))
        if t.dim() != 1 or t.numel() < 1:
            raise ValueError("expected 1-D F0 tracks of at least one frame, got %s" % (tuple(t.shape),))
        ts.append(t.to(dev, torch.float32))
    offs = np.zeros(len(ts) + 1, dtype=np.int64)
    np.cumsum([t.numel() for t in ts], out=offs[1:])
    return (torch.cat(ts) if len(ts) > 1 else ts[0]).contiguous(), offs


def f0_stats(f0_x, f0_y, paths):
    """F0 tracks (lists of [T_i], 0 = unvoiced) and the pairs' warping paths (list of int32 [length_p, 2], as ``dtw(..., return_path=True)``
    returns them) -> dict of numpy arrays over the pairs: ``rmse_cents``, ``bias_cents`` (float64; nan where ``voiced_pairs`` is 0),
    ``vuv_error``, ``voiced_pairs``, ``length``, and the raw ``counts`` [n, 4] (both voiced, x only, y only, neither).  One launch."""
    dev = _hip.hip_device("mask_cyclegan_vc.metrics")
    f0_x, f0_y, paths = list(f0_x), list(f0_y), list(paths)
    n = len(paths)
    if n < 1 or len(f0_x) != n or len(f0_y) != n:
        raise ValueError("f0_x, f0_y and paths must hold the same number (>= 1) of utterances, got %d, %d and %d" % (len(f0_x), len(f0_y), n))
    fx, xo = _tracks(f0_x, dev)
    fy, yo = _tracks(f0_y, dev)
    ps = []
    for k, p in enumerate(paths):
        t = p.detach() if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(p))
        if t.dim() != 2 or t.shape[1] != 2 or t.shape[0] < 1 or t.dtype not in (torch.int32, torch.int64):
            raise ValueError("path %d: expected integer [length, 2] rows, got %s %s" % (k, t.dtype, tuple(t.shape)))
        t = t.to(dev, torch.int32)
        lo, hi = t.amin(dim=0).cpu().numpy(), t.amax(dim=0).cpu().numpy()
        if lo.min() < 0 or hi[0] >= xo[k + 1] - xo[k] or hi[1] >= yo[k + 1] - yo[k]:
            raise ValueError("path %d leaves its utterances of %d and %d frames" % (k, xo[k + 1] - xo[k], yo[k + 1] - yo[k]))
        ps.append(t)
    po = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([t.shape[0] for t in ps], out=po[1:])
    table = np.stack([xo[:-1], yo[:-1], po[:-1], np.diff(po)], axis=1).astype(np.int64)
    with torch.no_grad(), torch.cuda.device(dev):
        path = (torch.cat(ps, dim=0) if n > 1 else ps[0]).contiguous()
        table_d = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
        counts = torch.empty(n, 4, dtype=torch.int32, device=dev)
        sums = torch.empty(n, 2, dtype=torch.float32, device=dev)
        _hip.check(_hip.lib().mcvc_f0_stats(_hip.ptr(fx), fx.numel(), _hip.ptr(fy), fy.numel(), _hip.ptr(path), _hip.ptr(table_d), n,
                                            _hip.ptr(counts), _hip.ptr(sums), _hip.stream()), "mcvc_f0_stats")
        counts, sums = counts.cpu().numpy(), sums.cpu().numpy().astype(np.float64)
    length = np.diff(po)
    voiced = counts[:, 0].astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        bias = np.where(voiced > 0, sums[:, 0] / voiced, np.nan)
        rmse = np.where(voiced > 0, np.sqrt(sums[:, 1] / voiced), np.nan)
    return {"rmse_cents": rmse, "bias_cents": bias, "vuv_error": (counts[:, 1] + counts[:, 2]).astype(np.float64) / length, "voiced_pairs": voiced,
            "length": length, "counts": counts}


def f0_distortion(conv_wavs, tgt_wavs, conv_mels, tgt_mels, n_cep=24, tracker=None):
    """F0 RMSE / bias (cents) and voiced/unvoiced error of converted against target utterances, aligned by the DTW over their mel cepstra
    (the alignment ``mcd`` scores): cepstra, DTW with paths, the F0 banks of both sides, the statistics -> the dict of ``f0_stats`` plus the
    tracks ``f0_converted`` / ``f0_target`` (lists of float32 numpy), ``lags`` and ``threshold``.  A waveform whose frame count differs
    from its mel's is a ValueError that names the utterance."""
    from .pitch import PitchTracker
    from data_preprocessing.audio2mel import num_frames
    conv_wavs, tgt_wavs, conv_mels, tgt_mels = list(conv_wavs), list(tgt_wavs), list(conv_mels), list(tgt_mels)
    n = len(conv_mels)
    if n < 1 or len(conv_wavs) != n or len(tgt_wavs) != n or len(tgt_mels) != n:
        raise ValueError("waveforms and mels of both sides must hold the same number (>= 1) of utterances, got %d, %d, %d and %d"
                         % (len(conv_wavs), len(tgt_wavs), n, len(tgt_mels)))
    for side, wavs, mels in (("converted", conv_wavs, conv_mels), ("target", tgt_wavs, tgt_mels)):
        for k, (w, m) in enumerate(zip(wavs, mels)):
            samples = int(np.prod(w.shape))
            if num_frames(samples) != m.shape[-1]:
                raise ValueError("utterance %d (%s): a waveform of %d samples has %d frames, its mel has %d"
                                 % (k, side, samples, num_frames(samples), m.shape[-1]))
    cx, xo = mel_cepstra(conv_mels, n_cep)
    cy, yo = mel_cepstra(tgt_mels, n_cep)
    _, _, paths = dtw((cx, xo), (cy, yo), scale=MCD_SCALE, return_path=True)
    tracker = PitchTracker(cx.device) if tracker is None else tracker
    fx = [f for f, _ in tracker.bank(conv_wavs)]
    fy = [f for f, _ in tracker.bank(tgt_wavs)]
    res = f0_stats(fx, fy, paths)
    res.update(f0_converted=fx, f0_target=fy, lags=tracker.lags, threshold=tracker.threshold)
    return res


def host_ms_table(n_fft):
    """cos(2 pi j / n_fft), j < n_fft, as a float32 host array (``mcvc_ms_table_init``)."""
    n_fft = _check_fft(n_fft)
    host = np.empty(n_fft, dtype=np.float32)
    _hip.check(_hip.lib().mcvc_ms_table_init(n_fft, host.ctypes.data), "mcvc_ms_table_init")
    return host


def _check_fft(n_fft):
    if isinstance(n_fft, bool) or int(n_fft) != n_fft or int(n_fft) not in MS_FFTS:
        raise ValueError("n_fft must be one of %s, got %r" % (", ".join(map(str, MS_FFTS)), n_fft))
    return int(n_fft)


def ms_bins(n_fft, max_hz=None):
    """-> (F, max_hz): the number of leading bins f = 1 .. F at or below ``max_hz`` (None: all n_fft / 2, up to Nyquist)."""
    n_fft = _check_fft(n_fft)
    nyquist = FRAME_RATE / 2.0
    if max_hz is None:
        return n_fft // 2, nyquist
    max_hz = float(max_hz)
    if not math.isfinite(max_hz) or max_hz > nyquist:
        raise ValueError("max_hz must not lie above Nyquist, %.2f Hz at %.2f frames per second, got %r" % (nyquist, FRAME_RATE, max_hz))
    F = int(math.floor(max_hz * n_fft / FRAME_RATE + 1e-9))
    if F < 1:
        raise ValueError("max_hz %r selects no bin: the first bin of n_fft %d lies at %.4f Hz" % (max_hz, n_fft, FRAME_RATE / n_fft))
    return min(F, n_fft // 2), max_hz


def modulation_spectrum(feats, n_fft=4096):
    """Ragged batch (list of [K, T_i], or ``(bank, offs)``) -> dict of device tensors ``power`` [n, K, n_fft / 2] (bin f at index f - 1),
    ``mean`` [n, K], ``var`` [n, K], plus ``offs`` and ``n_fft``; one launch on the current stream.  ``power`` takes 4 n K n_fft / 2 bytes:
    6.9 MB for 35 utterances at K = 24 and n_fft = 4096.  ValueError: an n_fft outside 1024 / 2048 / 4096, an utterance longer than n_fft,
    a bank that is not on the device, features that are not finite."""
    n_fft = _check_fft(n_fft)
    if isinstance(feats, tuple) and len(feats) == 2 and isinstance(feats[0], torch.Tensor) and not feats[0].is_cuda:
        raise ValueError("the bank of a (bank, offs) pair must live on a HIP device; there is no CPU path")
    b, offs = bank(feats)
    lens = np.diff(offs)
    if int(lens.max()) > n_fft:
        u = int(np.argmax(lens > n_fft))
        raise ValueError("utterance %d has %d frames, more than n_fft = %d: nothing is truncated" % (u, int(lens[u]), n_fft))
    dev, K, n = b.device, b.shape[0], len(lens)
    table = _hip.device_constant(("metrics.ms_table", n_fft), dev, lambda: host_ms_table(n_fft))
    with torch.no_grad(), torch.cuda.device(dev):
        offs_d = torch.from_numpy(offs).to(dev)
        power = torch.empty(n, K, n_fft // 2, dtype=torch.float32, device=dev)
        mean = torch.empty(n, K, dtype=torch.float32, device=dev)
        var = torch.empty(n, K, dtype=torch.float32, device=dev)
        _hip.check(_hip.lib().mcvc_ms_power(_hip.ptr(b), b.shape[1], K, _hip.ptr(offs_d), n, offs.ctypes.data, n_fft, _hip.ptr(table), _hip.ptr(power),
                                            _hip.ptr(mean), _hip.ptr(var), _hip.stream()), "mcvc_ms_power")
    return {"power": power, "mean": mean, "var": var, "offs": offs, "n_fft": n_fft}


def mean_log(values, floor=MS_FLOOR):
    """device [n, ...] -> device [...]: (1/n) sum_u 10 log10(max(values[u], floor)) in dB, utterances in index order; one launch."""
    floor = float(floor)
    if not (floor > 0.0 and math.isfinite(floor)):
        raise ValueError("floor must be positive and finite, got %r" % (floor,))
    dev = _hip.hip_device("mask_cyclegan_vc.metrics", values.device if isinstance(values, torch.Tensor) and values.is_cuda else None)
    _hip.require_on_device("mask_cyclegan_vc.metrics", values, dev, "values", "metrics")
    if values.dim() < 2 or values.shape[0] < 1 or values[0].numel() < 1:
        raise ValueError("expected [n, ...] values with n >= 1, got %s" % (tuple(values.shape),))
    v = values.detach().to(torch.float32).contiguous()
    with torch.no_grad(), torch.cuda.device(dev):
        out = torch.empty(v.shape[1:], dtype=torch.float32, device=dev)
        _hip.check(_hip.lib().mcvc_ms_mean_log(_hip.ptr(v), v.shape[0], out.numel(), floor, _hip.ptr(out), _hip.stream()), "mcvc_ms_mean_log")
    return out


def table_distance(a, b, n_used=None):
    """device tables [K, n_bins] (or [K]: one row of K bins) -> (per_dim [rows], total [1]) device tensors: the root mean square of a - b
    over the first ``n_used`` bins of every row and over all of them; one launch, one workgroup."""
    dev = _hip.hip_device("mask_cyclegan_vc.metrics", a.device if isinstance(a, torch.Tensor) and a.is_cuda else None)
    _hip.require_on_device("mask_cyclegan_vc.metrics", a, dev, "a", "metrics")
    _hip.require_on_device("mask_cyclegan_vc.metrics", b, dev, "b", "metrics")
    if a.shape != b.shape or a.dim() not in (1, 2):
        raise ValueError("expected two tables of one shape [K, n_bins] or [K], got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    a2 = a.detach().to(torch.float32).contiguous().reshape(1 if a.dim() == 1 else a.shape[0], -1)
    b2 = b.detach().to(torch.float32).contiguous().reshape(a2.shape)
    rows, n_bins = a2.shape
    n_used = n_bins if n_used is None else int(n_used)
    if not 1 <= rows <= MAX_K or not 1 <= n_bins <= MS_FFTS[-1] // 2 or not 1 <= n_used <= n_bins:
        raise ValueError("tables of 1 .. %d rows and 1 .. %d bins, 1 <= n_used <= n_bins; got %s, n_used %d" % (MAX_K, MS_FFTS[-1] // 2, tuple(a2.shape), n_used))
    with torch.no_grad(), torch.cuda.device(dev):
        per_dim = torch.empty(rows, dtype=torch.float32, device=dev)
        total = torch.empty(1, dtype=torch.float32, device=dev)
        _hip.check(_hip.lib().mcvc_ms_distance(_hip.ptr(a2), _hip.ptr(b2), rows, n_bins, n_used, _hip.ptr(per_dim), _hip.ptr(total), _hip.stream()),
                   "mcvc_ms_distance")
    return per_dim, total


def msd(converted_mels, target_mels, n_cep=24, n_fft=4096, max_hz=None):
    """Modulation-spectrum distance and global-variance distance (dB) between two SETS of log10-mels, which may differ in size and need not
    be parallel: cepstra, ``modulation_spectrum`` of both sets, the mean-log tables, the distances -- ``mcvc_ms_launches()`` = 8 launches after
    the two projections.  -> dict: ``msd``, ``gvd`` (floats), ``msd_per_dim`` [n_cep], ``lgv_converted`` / ``lgv_target`` [n_cep],
    ``lms_converted`` / ``lms_target`` [n_cep, n_fft / 2] (numpy), ``n_converted``, ``n_target``, ``n_fft``, ``n_bins_used``, ``max_hz``,
    ``floor``.  Each set's ``power`` array takes 4 n n_cep n_fft / 2 bytes on the device: 6.9 MB for 35 utterances at the defaults.
    ValueError: an utterance longer than n_fft, an n_fft outside 1024 / 2048 / 4096, a max_hz that selects no bin or lies above Nyquist."""
    F, hz = ms_bins(n_fft, max_hz)
    sides = []
    for mels in (converted_mels, target_mels):
        ms = modulation_spectrum(mel_cepstra(mels, n_cep), n_fft)
        sides.append((mean_log(ms["power"]), mean_log(ms["var"]), ms["power"].shape[0]))
    (lms_x, lgv_x, nx), (lms_y, lgv_y, ny) = sides
    per_dim, total = table_distance(lms_x, lms_y, F)
    _, gv = table_distance(lgv_x, lgv_y)
    return {"msd": float(total.cpu()[0]), "gvd": float(gv.cpu()[0]), "msd_per_dim": per_dim.cpu().numpy(),
            "lgv_converted": lgv_x.cpu().numpy(), "lgv_target": lgv_y.cpu().numpy(), "lms_converted": lms_x.cpu().numpy(), "lms_target": lms_y.cpu().numpy(),
            "n_converted": int(nx), "n_target": int(ny), "n_fft": int(n_fft), "n_bins_used": int(F), "max_hz": float(hz), "floor": MS_FLOOR}
