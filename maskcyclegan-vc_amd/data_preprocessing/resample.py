"""Sample-rate conversion on the GPU: ``scipy.signal.resample_poly``'s default filter, applied to a whole bank of utterances by one HIP
launch (csrc/resample_kernels.hip through ``mcvc_resample_run``).  There is no CPU path.

For rates ``r_in -> r_out`` with ``g = gcd(r_in, r_out)``, ``up = r_out / g``, ``down = r_in / g``, ``m = max(up, down)``, ``half = 10 m``:

* taps ``h = up * firwin(2 half + 1, 1 / m, window=('kaiser', 5.0))``: ``(1/m) sinc((n - half) / m) * kaiser(2 half + 1, 5.0)[n]``, scaled to
  sum 1, times ``up``; float64 here (``resample_taps``), rounded once to float32 for the device;
* ``n_out = ceil(n_in * up / down)``;
* ``y[k] = sum_i x[i] h[k down + half - i up]`` over the ``i`` in ``[0, n_in)`` whose tap index lies in ``[0, 2 half]``: samples outside the
  utterance count as zero (``padtype='constant'``).

It is NOT librosa's resampler (soxr / resampy): a file at another rate gives close but not identical samples to the reference's
``librosa.load(path, sr=22050)``.  ``max(up, down)`` is at most ``mcvc_resample_max_factor()`` = 640, which covers every pair between 22050 Hz
and 8000, 11025, 12000, 16000, 24000, 32000, 44100, 48000, 88200 and 96000 Hz.
"""
import ctypes
from math import gcd

import numpy as np

MAX_FACTOR = 640                                                       # mcvc_resample_max_factor()
_NAME = "data_preprocessing.resample"


def ratio(rate_in, rate_out):
    """-> (up, down) in lowest terms."""
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in < 1 or rate_out < 1:
        raise ValueError("sample rates must be positive, got %d -> %d" % (rate_in, rate_out))
    g = gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g


def resample_taps(up, down):
    """The float64 taps ``up * firwin(20 max(up, down) + 1, 1 / max(up, down), window=('kaiser', 5.0))``, from numpy alone."""
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError("up and down must be positive, got %d / %d" % (up, down))
    m = max(up, down)
    half = 10 * m
    n = np.arange(2 * half + 1, dtype=np.float64) - half
    h = (1.0 / m) * np.sinc(n / m) * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * up


def out_samples(n_in, up, down):
    return -((-int(n_in) * int(up)) // int(down))


def _check_factors(up, down):
    if max(up, down) > MAX_FACTOR:
        raise ValueError("%s (MI355X build): max(up, down) = %d is beyond the kernel's limit of %d (rates %d/%d in lowest terms)"
                         % (_NAME, max(up, down), MAX_FACTOR, up, down))


class Resampler(object):
    """``rs.bank(waveforms, rate_in, rate_out)`` for utterances of different lengths (one upload, one launch) and
    ``rs(x, rate_in, rate_out)`` for a HIP-device tensor [B, L] -> [B, ceil(L up / down)]."""

    def __init__(self, device=None):
        from mask_cyclegan_vc._hip import hip_device
        self.device = hip_device(_NAME, device)
        self._in_flight = []                                           # (event, pinned work list): kept until the launch that reads it is done

    def table(self, up, down):
        """The packed polyphase table (``mcvc_resample_pack``), uploaded once per (up, down, device)."""
        from mask_cyclegan_vc._hip import check, device_constant, lib
        _check_factors(up, down)

        def host_table():
            L = lib()
            h = np.ascontiguousarray(resample_taps(up, down), dtype=np.float32)
            host = np.empty(L.mcvc_resample_table_floats(up, down), dtype=np.float32)
            check(L.mcvc_resample_pack(h.ctypes.data, h.size, up, down, host.ctypes.data), "mcvc_resample_pack")
            return host
        return device_constant("resample.table.%d.%d" % (up, down), self.device, host_table)

    def launch(self, wave, lengths, up, down):
        """wave: contiguous float32 device tensor holding the utterances back to back -> (resampled device bank, int32 output offsets)."""
        import torch
        from mask_cyclegan_vc._hip import check, lib, ptr, require_on_device, stream
        require_on_device(_NAME, wave, self.device, "waveform bank", "resampler")
        _check_factors(up, down)
        L = lib()
        n = len(lengths)
        offs = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.asarray(lengths, dtype=np.int64), out=offs[1:])
        if n < 1 or offs[-1] >= 2 ** 31 or min(lengths) < 1 or wave.numel() != offs[-1] or wave.dtype != torch.float32 or not wave.is_contiguous():
            raise ValueError("a bank holds between 1 utterance and 2^31 - 1 samples, none empty, as one contiguous float32 buffer")
        offs = offs.astype(np.int32)
        out_offs = np.zeros(n + 1, dtype=np.int32)
        n_tiles = ctypes.c_int(0)
        check(L.mcvc_resample_plan(offs.ctypes.data, n, up, down, out_offs.ctypes.data, None, 0, ctypes.byref(n_tiles)), "mcvc_resample_plan")
        tiles = torch.empty(n_tiles.value, 8, dtype=torch.int32).pin_memory()      # read by the host check and, mapped, by the kernel
        check(L.mcvc_resample_plan(offs.ctypes.data, n, up, down, out_offs.ctypes.data, tiles.data_ptr(), n_tiles.value, ctypes.byref(n_tiles)),
              "mcvc_resample_plan")
        total = int(out_offs[-1])
        self._in_flight = [(e, t) for e, t in self._in_flight if not e.query()]
        with torch.cuda.device(self.device):
            out = torch.empty(total, dtype=torch.float32, device=self.device)
            check(L.mcvc_resample_run(ptr(wave), int(offs[-1]), ctypes.c_void_p(tiles.data_ptr()), n_tiles.value, ptr(self.table(up, down)), up, down,
                                      ptr(out), total, stream()), "mcvc_resample_run")
            done = torch.cuda.Event()
            done.record()
        self._in_flight.append((done, tiles))
        return out, out_offs

    def bank(self, waveforms, rate_in, rate_out, to_host=False):
        """list of 1-D waveforms (numpy or tensors, host or device) -> (float32 device bank, int32 offsets [n + 1]) at ``rate_out``, or a
        list of float32 numpy arrays with ``to_host=True``.  Equal rates: the bank as it came, no launch."""
        import torch
        up, down = ratio(rate_in, rate_out)
        _check_factors(up, down)
        if not len(waveforms):
            raise ValueError("a bank holds at least one utterance")
        if all(isinstance(w, torch.Tensor) and w.is_cuda for w in waveforms):
            parts = [w.to(self.device, torch.float32).reshape(-1) for w in waveforms]
            lengths = [int(p.numel()) for p in parts]
            wave = torch.cat(parts) if len(parts) > 1 else parts[0].contiguous()
        else:
            ws = [np.ascontiguousarray(w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w, dtype=np.float32).reshape(-1) for w in waveforms]
            lengths = [w.size for w in ws]
            wave = torch.from_numpy(np.concatenate(ws)).to(self.device)
        if up == down:
            out, offs = wave, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        else:
            out, offs = self.launch(wave, lengths, up, down)
        if not to_host:
            return out, offs
        host = out.cpu().numpy()
        return [np.ascontiguousarray(host[offs[i]:offs[i + 1]]) for i in range(len(lengths))]

    def __call__(self, x, rate_in, rate_out):
        import torch
        from mask_cyclegan_vc._hip import require_on_device
        require_on_device(_NAME, x, self.device, "waveform", "resampler")
        if x.dim() != 2:
            raise ValueError("expected a [B, L] waveform tensor, got %s" % (tuple(x.shape),))
        up, down = ratio(rate_in, rate_out)
        _check_factors(up, down)
        if up == down:
            return x
        B, n = x.shape
        out, _ = self.launch(x.to(torch.float32).contiguous().view(-1), [n] * B, up, down)
        return out.view(B, out_samples(n, up, down))
