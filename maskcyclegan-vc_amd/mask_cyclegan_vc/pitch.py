"""Pitch tracking on the HIP kernels: F0 contours of a bank of utterances in one launch (csrc/f0_kernels.hip through ``mcvc_f0_track``).
All arithmetic runs in the kernel; Python builds tables and moves data.  There is no CPU path.  New: the reference has no F0 anywhere.

The tracker is YIN (de Cheveigne & Kawahara 2002); tests/f0_checker.py restates it in float64.

Frame grid.  22050 Hz, hop 256, integration window W = 1024.  Frames are the mel front-end's: an utterance of L >= 385 samples has
T = (L - 256) // 256 + 1 frames, and frame t is centred on sample c_t = 256 t + 128, the centre of mel frame t's window in un-padded
coordinates.  F0 frame t and mel column t describe the same instant, so a DTW path over mel cepstra indexes F0 tracks directly.  Frames
and the launch's work list come from ``mcvc_audio_plan``, the front-end's own.

Lag range.  tau_min = ceil(22050 / fmax), tau_max = floor(22050 / fmin), computed here; 2 <= tau_min < tau_max <= 640 (34.5 Hz).  The
defaults fmin 60, fmax 500 give 45 .. 367.

Difference function.  s = c_t - (W + tau_max) // 2 (it may be negative), buf[j] = x[s + j] for 0 <= j < W + tau_max, zero outside
[0, L) of the same utterance; d(tau) = sum_{j < W} (buf[j] - buf[j + tau])^2, computed from the differences (never as energy minus
autocorrelation: its cancellation destroys the small values the decisions are made on).

Normalisation.  d'(0) = 1, d'(tau) = d(tau) tau / sum_{1 <= k <= tau} d(k), and 1 where that sum is 0 (digital silence, DC).

Pick.  Scan tau = tau_min .. tau_max upward; at the first tau with d'(tau) < threshold (default 0.15) descend: while tau + 1 <= tau_max
and d'(tau + 1) < d'(tau), tau += 1.  Every comparison is strict and made on the stored float32 values.  With a, b, c = d'(tau - 1),
d'(tau), d'(tau + 1): off = 0 at tau_max, else den = (a - b) + (c - b) and off = clamp(0.5 (a - c) / den, -0.5, 0.5) where den > 0, else 0.
f0 = 22050 / (tau + off) (it may leave [fmin, fmax] by a fraction of a lag: not clamped), aperiodicity = b.  No lag under the threshold:
f0 = 0 (unvoiced) and aperiodicity = min d' over the range.

A bank equals its single calls bit for bit: a frame sees only its own utterance, and its sums have one order.
"""
import math

import numpy as np
import torch

from . import _hip

SAMPLING_RATE = 22050
HOP_LENGTH = 256
WINDOW = 1024
MAX_LAG = 640                                                          # mcvc_f0_max_lag()


def lag_range(fmin, fmax):
    """(tau_min, tau_max) of a frequency range in Hz; raises ValueError for a range the kernel does not take."""
    fmin, fmax = float(fmin), float(fmax)
    if not (math.isfinite(fmin) and math.isfinite(fmax) and 0.0 < fmin < fmax):
        raise ValueError("the F0 range needs 0 < fmin < fmax, got %r .. %r Hz" % (fmin, fmax))
    tau_min, tau_max = int(math.ceil(SAMPLING_RATE / fmax)), int(math.floor(SAMPLING_RATE / fmin))
    if not 2 <= tau_min < tau_max <= MAX_LAG:
        raise ValueError("%g .. %g Hz are the lags %d .. %d; the tracker takes 2 <= tau_min < tau_max <= %d (%.1f Hz .. %g Hz)"
                         % (fmin, fmax, tau_min, tau_max, MAX_LAG, SAMPLING_RATE / MAX_LAG, SAMPLING_RATE / 2.0))
    return tau_min, tau_max


def check_threshold(threshold):
    threshold = float(threshold)
    if not (math.isfinite(threshold) and 0.0 < threshold <= 1.0):
        raise ValueError("the YIN threshold lies in (0, 1], got %r" % (threshold,))
    return threshold


class PitchTracker(object):
    """``PitchTracker().bank(waveforms)`` -> [(f0, aperiodicity)] float32 numpy [T_i] per utterance from one launch; f0 = 0 marks an
    unvoiced frame.  ``track`` is the same on device tensors."""

    def __init__(self, device=None, fmin=60.0, fmax=500.0, threshold=0.15):
        self.fmin, self.fmax = float(fmin), float(fmax)
        self._lags = lag_range(fmin, fmax)
        self.threshold = check_threshold(threshold)
        self.device = _hip.hip_device("mask_cyclegan_vc.metrics", device)                # (the name these messages have always carried)

    @property
    def lags(self):
        return self._lags

    def track(self, wave, lengths, return_cmnd=False):
        """wave: contiguous float32 device tensor holding the utterances back to back; lengths: their sample counts.
        -> (f0 [N], aperiodicity [N], frame_offs int32 numpy [n + 1][, cmnd [tau_max + 1, N]]) on the current stream; utterance u owns
        frames frame_offs[u] .. frame_offs[u + 1].  ``cmnd`` holds the d' values the pick was made on."""
        from data_preprocessing.audio2mel import plan_bank
        _hip.require_on_device("mask_cyclegan_vc.pitch", wave, self.device, "waveform", "tracker")
        if wave.dtype != torch.float32 or not wave.is_contiguous() or wave.dim() != 1:
            raise ValueError("expected a contiguous 1-D float32 tensor of samples")
        lengths = [int(k) for k in lengths]
        offs, frame_offs, tiles = plan_bank(lengths)
        if offs[-1] != wave.numel():
            raise ValueError("the lengths add up to %d samples, the tensor holds %d" % (offs[-1], wave.numel()))
        L = _hip.lib()
        total = int(frame_offs[-1])
        tau_min, tau_max = self._lags
        with torch.no_grad(), torch.cuda.device(self.device):
            tiles_d = torch.from_numpy(tiles).to(self.device)
            f0 = torch.empty(total, dtype=torch.float32, device=self.device)
            ap = torch.empty(total, dtype=torch.float32, device=self.device)
            cm = torch.empty(tau_max + 1, total, dtype=torch.float32, device=self.device) if return_cmnd else None
            _hip.check(L.mcvc_f0_track(_hip.ptr(wave), int(offs[-1]), _hip.ptr(tiles_d), tiles.shape[0], tau_min, tau_max, self.threshold,
                                       _hip.ptr(f0), _hip.ptr(ap), _hip.ptr(cm), total, _hip.stream()), "mcvc_f0_track")
        return (f0, ap, frame_offs, cm) if return_cmnd else (f0, ap, frame_offs)

    def bank(self, waveforms):
        """list of 1-D waveforms (numpy or tensors, any float type) -> list of (f0, aperiodicity) float32 numpy [T_i], from a single launch."""
        from data_preprocessing.audio2mel import num_frames
        ws = [np.ascontiguousarray(w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w, dtype=np.float32).reshape(-1) for w in waveforms]
        if not ws:
            return []
        for i, w in enumerate(ws):
            num_frames(w.size)
            if not np.isfinite(w).all():
                raise ValueError("waveform %d holds samples that are not finite" % i)
        f0, ap, fo = self.track(torch.from_numpy(np.concatenate(ws)).to(self.device), [w.size for w in ws])
        f0, ap = f0.cpu().numpy(), ap.cpu().numpy()
        return [(np.ascontiguousarray(f0[fo[i]:fo[i + 1]]), np.ascontiguousarray(ap[fo[i]:fo[i + 1]])) for i in range(len(ws))]
