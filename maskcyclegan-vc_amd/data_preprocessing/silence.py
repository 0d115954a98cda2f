"""Silence detection on the GPU: where an utterance starts and ends, and where a long recording can be cut.  The definition is
``librosa.effects.trim`` / ``librosa.effects.split`` as published (``frame_length=2048``, ``hop_length=512``, ``ref=np.max``), restated; librosa
is not a dependency and the results are NOT verified against librosa.

For one utterance of ``L >= 1`` samples at 22050 Hz:

* ``T = 1 + L // 512`` frames; frame ``t`` covers samples ``[512 t - 1024, 512 t + 1024)``, zero outside ``[0, L)`` of the same utterance;
* ``mse[t] = (1 / 2048) sum x^2`` in float32, ``ref = max_t mse[t]``: one HIP launch for a whole ragged bank (csrc/vad_kernels.hip through
  ``mcvc_vad_energy``).  There is no CPU path;
* frame ``t`` is non-silent iff ``max(mse[t], 1e-10f) > max(ref, 1e-10f) * r`` with ``r = float32(10 ** (-top_db / 10))``: one float32 product
  and one strict compare, on the host (``nonsilent``), never on a logarithm.  ``top_db`` is finite and > 0, so the loudest frame is always
  non-silent; an all-zero utterance has ``ref = 0``, every frame non-silent, and comes back whole, as librosa returns it;
* ``frame_db``: ``10 log10(max(mse, 1e-10)) - 10 log10(max(ref, 1e-10))``, for reports only;
* trim: ``(512 first, min(L, 512 (last + 1)))`` of the first and last non-silent frame;
* split: each maximal run ``[a, b]`` of non-silent frames gives ``[512 a, min(L, 512 (b + 1)))``; consecutive intervals whose gap is under
  ``round(min_silence_ms * 22.05)`` samples are joined (``merge_intervals``); then intervals under 16384 samples -- 64 mel frames, the
  training crop -- are dropped and counted (``drop_short``).

Frame length and hop are fixed.  ``Audio2Mel.bank(..., trim_db=)``, ``bank_at_rates(..., trim_db=)`` and ``bank_split`` detect on the 22050 Hz
device bank and run the log-mel launch over the segments in place (data_preprocessing/audio2mel.py).
"""
import ctypes
import math

import numpy as np

FRAME_LENGTH = 2048                                                    # mcvc_vad_frame_length()
HOP = 512                                                              # mcvc_vad_hop()
AMIN = np.float32(1e-10)
MIN_SEGMENT = 16384                                                    # 64 mel frames: preprocess_vcc2018.MIN_FRAMES * audio2mel.HOP_LENGTH
SAMPLES_PER_MS = 22.05
_NAME = "data_preprocessing.silence"


def num_frames(n_samples):
    return 1 + int(n_samples) // HOP


def threshold_ratio(top_db):
    """``float32(10 ** (-top_db / 10))``, formed in float64 and rounded once.  Raises unless ``top_db`` is finite and > 0."""
    top_db = float(top_db)
    if not math.isfinite(top_db) or top_db <= 0.0:
        raise ValueError("top_db must be finite and > 0, got %r" % top_db)
    return np.float32(10.0 ** (-top_db / 10.0))


def nonsilent(mse, ref, top_db):
    """-> bool [T]: the decision of the module docstring in float32 (one product, one strict compare)."""
    r = threshold_ratio(top_db)
    mse = np.asarray(mse, dtype=np.float32)
    level = np.maximum(np.float32(ref), AMIN) * r
    assert level.dtype == np.float32
    return np.maximum(mse, AMIN) > level


def frame_db(mse, ref):
    """dB of every frame under the loudest one (<= 0), float64: for reports, never for decisions."""
    mse = np.asarray(mse, dtype=np.float32)
    return 10.0 * np.log10(np.maximum(mse, AMIN).astype(np.float64)) - 10.0 * np.log10(float(max(np.float32(ref), AMIN)))


def trim_bounds(flags, n_samples):
    idx = np.flatnonzero(flags)
    if idx.size == 0:
        raise ValueError("no non-silent frame: the loudest frame always is one (were the energies and ref of the same utterance?)")
    return int(HOP * idx[0]), int(min(int(n_samples), HOP * (idx[-1] + 1)))


def split_intervals(flags, n_samples):
    """Maximal runs of non-silent frames -> [(start, end)] in samples, in order, none empty."""
    f = np.concatenate([[False], np.asarray(flags, dtype=bool), [False]])
    edges = np.flatnonzero(f[1:] != f[:-1])                            # run k is frames [edges[2k], edges[2k + 1])
    return [(int(HOP * a), int(min(int(n_samples), HOP * b))) for a, b in zip(edges[0::2], edges[1::2])]


def gap_samples(min_silence_ms):
    min_silence_ms = float(min_silence_ms)
    if not math.isfinite(min_silence_ms) or min_silence_ms < 0.0:
        raise ValueError("min_silence_ms must be finite and >= 0, got %r" % min_silence_ms)
    return int(round(min_silence_ms * SAMPLES_PER_MS))


def merge_intervals(intervals, min_silence_ms):
    """Consecutive intervals whose gap ``s[k + 1] - e[k]`` is under ``round(min_silence_ms * 22.05)`` samples are joined."""
    G = gap_samples(min_silence_ms)
    out = []
    for s, e in intervals:
        if out and s - out[-1][1] < G:
            out[-1] = (out[-1][0], e)
        else:
            out.append((int(s), int(e)))
    return out


def drop_short(intervals, min_samples=MIN_SEGMENT):
    """-> (intervals of at least ``min_samples`` samples, number dropped)."""
    kept = [(s, e) for s, e in intervals if e - s >= min_samples]
    return kept, len(intervals) - len(kept)


class SilenceDetector(object):
    """``det.energies(waveforms)`` -> frame energies and their maxima from one upload and ``mcvc_vad_launches()`` launches; ``nonsilent``,
    ``frame_db``, ``trim`` and ``split`` are host logic on those values."""

    def __init__(self, device=None):
        from mask_cyclegan_vc._hip import hip_device
        self.device = hip_device(_NAME, device)

    nonsilent = staticmethod(nonsilent)
    frame_db = staticmethod(frame_db)

    def launch(self, wave, lengths):
        """wave: contiguous float32 device tensor holding the utterances back to back -> (mse device [total_frames], ref device [n],
        int32 frame offsets [n + 1])."""
        import torch
        from mask_cyclegan_vc._hip import check, lib, ptr, require_on_device, stream
        require_on_device(_NAME, wave, self.device, "waveform bank", "silence detector")
        L = lib()
        n = len(lengths)
        offs = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.asarray(lengths, dtype=np.int64), out=offs[1:])
        if n < 1 or offs[-1] >= 2 ** 31 or min(lengths) < 1 or wave.numel() != offs[-1] or wave.dtype != torch.float32 or not wave.is_contiguous():
            raise ValueError("a bank holds between 1 utterance and 2^31 - 1 samples, none empty, as one contiguous float32 buffer")
        offs = offs.astype(np.int32)
        frame_offs = np.zeros(n + 1, dtype=np.int32)
        n_tiles = ctypes.c_int(0)
        check(L.mcvc_vad_plan(offs.ctypes.data, n, frame_offs.ctypes.data, None, 0, ctypes.byref(n_tiles)), "mcvc_vad_plan")
        tiles = np.zeros((n_tiles.value, 4), dtype=np.int32)
        check(L.mcvc_vad_plan(offs.ctypes.data, n, frame_offs.ctypes.data, tiles.ctypes.data, n_tiles.value, ctypes.byref(n_tiles)), "mcvc_vad_plan")
        total = int(frame_offs[-1])
        with torch.cuda.device(self.device):
            tables = torch.from_numpy(np.concatenate([tiles.reshape(-1), frame_offs])).to(self.device)     # one upload: work list | frame offsets
            tiles_d, fo_d = tables[:tiles.size], tables[tiles.size:]
            out = torch.empty(total + n, dtype=torch.float32, device=self.device)                         # mse | ref: one download
            mse, ref = out[:total], out[total:]
            check(L.mcvc_vad_energy(ptr(wave), int(offs[-1]), ptr(tiles_d), n_tiles.value, ptr(fo_d), n, ptr(mse), total, ptr(ref), stream()),
                  "mcvc_vad_energy")
        return out, total, frame_offs

    def energies(self, waveforms, lengths=None):
        """``waveforms``: a list of 1-D host arrays (any float type), or -- with ``lengths`` -- a contiguous float32 device tensor that holds
        the utterances back to back.  -> (list of float32 numpy [T_i], float32 numpy [n])."""
        import torch
        if lengths is None:
            ws = [np.ascontiguousarray(w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w, dtype=np.float32).reshape(-1) for w in waveforms]
            if not ws:
                raise ValueError("a bank holds at least one utterance")
            lengths = [w.size for w in ws]
            if min(lengths) < 1:
                raise ValueError("an utterance holds at least one sample")
            wave = torch.from_numpy(np.concatenate(ws)).to(self.device)
        else:
            wave = waveforms
            lengths = [int(k) for k in lengths]
        out, total, fo = self.launch(wave, lengths)
        host = out.cpu().numpy()
        return [np.ascontiguousarray(host[fo[i]:fo[i + 1]]) for i in range(len(lengths))], np.ascontiguousarray(host[total:])

    def trim(self, waveforms, top_db, lengths=None):
        """-> [(start, end)] per utterance, in samples of that utterance."""
        threshold_ratio(top_db)
        mse, ref = self.energies(waveforms, lengths)
        lengths = [np.asarray(w).size for w in waveforms] if lengths is None else lengths
        return [trim_bounds(nonsilent(m, r, top_db), n) for m, r, n in zip(mse, ref, lengths)]

    def split(self, waveforms, top_db, min_silence_ms=300.0, lengths=None, min_samples=MIN_SEGMENT, return_dropped=False):
        """-> [[(start, end), ...]] per utterance: the non-silent runs, merged over gaps under ``min_silence_ms``, without the intervals
        under ``min_samples`` samples (``return_dropped``: and how many of those each utterance had)."""
        threshold_ratio(top_db)
        gap_samples(min_silence_ms)
        mse, ref = self.energies(waveforms, lengths)
        lengths = [np.asarray(w).size for w in waveforms] if lengths is None else lengths
        kept, dropped = [], []
        for m, r, n in zip(mse, ref, lengths):
            k, d = drop_short(merge_intervals(split_intervals(nonsilent(m, r, top_db), n), min_silence_ms), min_samples)
            kept.append(k)
            dropped.append(d)
        return (kept, dropped) if return_dropped else kept
