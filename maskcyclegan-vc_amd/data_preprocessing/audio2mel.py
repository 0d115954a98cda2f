"""Waveform -> log-mel front-end on the GPU: the MelGAN vocoder's ``Audio2Mel`` transform, which the reference obtains through
``torch.hub`` (data_preprocessing/preprocess_vcc2018.py:26-60, mask_cyclegan_vc/utils.py) and this project restates from its
published definition -- no network access, no trained weights, no librosa / torchaudio.

``Audio2Mel(n_fft=1024, hop_length=256, win_length=1024, sampling_rate=22050, n_mel_channels=80, mel_fmin=0.0, mel_fmax=None)``
on one mono float waveform of L samples:

1. reflect-pad (1024 - 256) / 2 = 384 samples each side (``F.pad(..., 'reflect')``: the edge sample is not repeated; L >= 385);
2. T = (L - 256) // 256 + 1 frames, frame t = padded samples [256 t, 256 t + 1024) (``center=False``);
3. periodic Hann window of 1024, DFT, bins 0..512, magnitude sqrt(re^2 + im^2);
4. mel = B @ magnitude with the [80, 513] Slaney filterbank of ``mel_filterbank`` (what ``librosa.filters.mel(sr=22050, n_fft=1024,
   n_mels=80, fmin=0, fmax=11025, htk=False, norm='slaney')`` is defined to return);
5. log10(clamp(mel, min=1e-5)), float32 [80, T].

Steps 1-5 are ONE HIP launch for a whole bank of utterances (csrc/audio_kernels.hip through ``mcvc_audio_log_mel``): a speaker's
recordings are concatenated in one buffer with an offset table and come back as one [80, total_frames] matrix.  There is no CPU path.

``read_wav`` follows ``librosa.load(path, sr=22050, mono=True)``: integer PCM scaled by 1 / 2^(bits-1), channels averaged; a file at
another rate is resampled on the host with ``scipy.signal.resample_poly`` -- NOT librosa's resampler (soxr / resampy), so such files
give close but not identical samples.  VCC2018 is recorded at 22050 Hz and never takes that branch.  ``read_wav_native`` stops before
that branch and ``Audio2Mel.bank_at_rates`` applies the same filter on the device instead (data_preprocessing/resample.py).
"""
import ctypes
from math import gcd

import numpy as np

SAMPLING_RATE = 22050
N_FFT = 1024
HOP_LENGTH = 256
N_MEL = 80
MIN_SAMPLES = (N_FFT - HOP_LENGTH) // 2 + 1        # reflect padding of 384 needs at least 385 samples


def num_frames(n_samples):
    """Frames of an utterance of ``n_samples`` samples; raises below 385 samples like torch's reflect padding."""
    n_samples = int(n_samples)
    if n_samples < MIN_SAMPLES:
        raise ValueError("Audio2Mel needs at least %d samples (reflect padding of %d), got %d" % (MIN_SAMPLES, MIN_SAMPLES - 1, n_samples))
    return (n_samples - HOP_LENGTH) // HOP_LENGTH + 1


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), f / (200.0 / 3.0))


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_filterbank(dtype=np.float32):
    """The [80, 513] Slaney mel basis (triangles between 82 band edges equally spaced on the Slaney mel scale from 0 to 11025 Hz,
    each scaled by 2 / its width in Hz), built in float64 and returned as ``dtype``."""
    fmax = SAMPLING_RATE / 2.0
    f = np.linspace(0.0, fmax, N_FFT // 2 + 1)
    e = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(fmax), N_MEL + 2))
    up = (f[None, :] - e[:-2, None]) / (e[1:-1] - e[:-2])[:, None]
    down = (e[2:, None] - f[None, :]) / (e[2:] - e[1:-1])[:, None]
    basis = np.maximum(0.0, np.minimum(up, down)) * (2.0 / (e[2:] - e[:-2]))[:, None]
    return basis.astype(dtype)


def _to_float(data):
    if data.dtype.kind == "f":
        return data.astype(np.float32)
    if data.dtype == np.uint8:                                         # 8-bit PCM is unsigned, centred on 128
        return (data.astype(np.float32) - 128.0) / 128.0
    if data.dtype.kind == "i":
        return (data.astype(np.float64) / float(1 << (8 * data.dtype.itemsize - 1))).astype(np.float32)
    raise ValueError("unsupported sample type %s" % data.dtype)


def _read_with_wave_module(path):
    import wave
    try:
        with wave.open(path, "rb") as fh:                              # the stdlib reader knows uncompressed PCM only
            rate, width, ch, n = fh.getframerate(), fh.getsampwidth(), fh.getnchannels(), fh.getnframes()
            raw = fh.readframes(n)
    except (wave.Error, EOFError) as exc:
        raise ValueError("%s: not a readable uncompressed PCM .wav file (%s)" % (path, exc))
    if width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        data = ((b[:, 0] << 8) | (b[:, 1] << 16) | (b[:, 2] << 24)).astype(np.int32)
    elif width in (1, 2, 4):
        data = np.frombuffer(raw, dtype={1: np.uint8, 2: "<i2", 4: "<i4"}[width])
    else:
        raise ValueError("%s: unsupported sample width of %d bytes" % (path, width))
    return rate, data.reshape(-1, ch) if ch > 1 else data


def read_wav_native(path):
    """-> (rate, float32 mono waveform at the file's own rate): ``read_wav`` before its resampling branch.  Raises ValueError for
    compressed, empty or unreadable files."""
    path = str(path)
    try:
        from scipy.io import wavfile
    except ImportError:
        wavfile = None
    if wavfile is not None:
        import warnings
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                        # (non-audio chunks in the header are not an error)
                rate, data = wavfile.read(path)
        except FileNotFoundError:
            raise
        except Exception as exc:                                       # scipy raises ValueError for formats it does not decode
            raise ValueError("%s: not a readable uncompressed .wav file (%s)" % (path, exc))
    else:
        rate, data = _read_with_wave_module(path)
    x = _to_float(np.asarray(data))
    if x.ndim == 2:
        x = x.mean(axis=1, dtype=np.float32)
    if x.size == 0:
        raise ValueError("%s: no samples" % path)
    return int(rate), x


def read_wav(path, sampling_rate=SAMPLING_RATE):
    """-> float32 mono waveform at ``sampling_rate`` (22050 Hz), like ``librosa.load(path, sr=22050, mono=True)`` except for the
    resampler (module docstring).  Raises ValueError for compressed, empty or unreadable files."""
    rate, x = read_wav_native(path)
    if int(rate) != int(sampling_rate):
        from scipy.signal import resample_poly
        g = gcd(int(sampling_rate), int(rate))
        x = resample_poly(x.astype(np.float64), int(sampling_rate) // g, int(rate) // g)
    return np.ascontiguousarray(x, dtype=np.float32)


def plan_bank(lengths):
    """Sample counts of a bank's utterances -> (sample offsets [n + 1], frame offsets [n + 1], the launch's work list [n_tiles, 4]) as int32
    numpy, through ``mcvc_audio_plan``: the frame grid every kernel that works on waveform banks shares."""
    from mask_cyclegan_vc._hip import check, lib
    L = lib()
    n = len(lengths)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.asarray(lengths, dtype=np.int64), out=offs[1:])
    if n < 1 or offs[-1] >= 2 ** 31:
        raise ValueError("a bank holds between 1 utterance and 2^31 - 1 samples")
    for k in lengths:
        num_frames(k)                                                  # raises for an utterance under 385 samples
    offs = offs.astype(np.int32)
    frame_offs = np.zeros(n + 1, dtype=np.int32)
    n_tiles = ctypes.c_int(0)
    check(L.mcvc_audio_plan(offs.ctypes.data, n, frame_offs.ctypes.data, None, 0, ctypes.byref(n_tiles)), "mcvc_audio_plan")
    tiles = np.zeros((n_tiles.value, 4), dtype=np.int32)
    check(L.mcvc_audio_plan(offs.ctypes.data, n, frame_offs.ctypes.data, tiles.ctypes.data, n_tiles.value, ctypes.byref(n_tiles)), "mcvc_audio_plan")
    return offs, frame_offs, tiles


class Audio2Mel(object):
    """The vocoder's front-end as a callable: ``fft(x)`` with ``x`` a HIP-device tensor [B, 1, L] or [B, L] -> [B, 80, T]
    (the convention of the reference's ``vocoder.fft``), and ``fft.bank(waveforms)`` for utterances of different lengths:
    one launch, one float32 [80, T_i] array per utterance."""

    def __init__(self, device=None):
        from mask_cyclegan_vc._hip import hip_device
        self.device = hip_device("data_preprocessing.audio2mel", device)

    def basis(self):
        """The constant operand (``mcvc_audio_basis_init``), uploaded once per device."""
        from mask_cyclegan_vc._hip import check, device_constant, lib

        def host_basis():
            L = lib()
            host = np.empty(L.mcvc_audio_basis_floats(), dtype=np.float32)
            check(L.mcvc_audio_basis_init(host.ctypes.data), "mcvc_audio_basis_init")
            return host
        return device_constant("audio2mel.basis", self.device, host_basis)

    def _launch(self, wave, lengths):
        """wave: contiguous float32 device tensor holding the utterances back to back -> ([80, total_frames] device tensor, frame offsets)."""
        import torch
        from mask_cyclegan_vc._hip import check, lib, ptr, stream
        offs, frame_offs, tiles = plan_bank(lengths)
        total = int(frame_offs[-1])
        with torch.cuda.device(self.device):
            tiles_d = torch.from_numpy(tiles).to(self.device)
            out = torch.empty(N_MEL, total, dtype=torch.float32, device=self.device)
            check(lib().mcvc_audio_log_mel(ptr(wave), int(offs[-1]), ptr(tiles_d), tiles.shape[0], ptr(self.basis()), ptr(out), total, stream()),
                  "mcvc_audio_log_mel")
        return out, frame_offs

    def _launch_segments(self, wave, starts, lengths):
        """``_launch`` for segments that lie anywhere in the bank ``wave``: segment i is samples [starts[i], starts[i] + lengths[i]),
        reflect-padded at its own ends (``mcvc_audio_plan_segments``; the kernel is the same).  Nothing is copied on the device."""
        import torch
        from mask_cyclegan_vc._hip import check, lib, ptr, stream
        L = lib()
        n = len(lengths)
        if n < 1 or len(starts) != n:
            raise ValueError("%d segment starts but %d lengths (at least one segment)" % (len(starts), n))
        for k in lengths:
            num_frames(k)                                              # raises for a segment under 385 samples
        if min(starts) < 0 or max(int(s) + int(k) for s, k in zip(starts, lengths)) > wave.numel():
            raise ValueError("a segment reaches outside the bank of %d samples" % wave.numel())
        st, ln = np.asarray(starts, dtype=np.int32), np.asarray(lengths, dtype=np.int32)
        frame_offs = np.zeros(n + 1, dtype=np.int32)
        n_tiles = ctypes.c_int(0)
        check(L.mcvc_audio_plan_segments(st.ctypes.data, ln.ctypes.data, n, frame_offs.ctypes.data, None, 0, ctypes.byref(n_tiles)), "mcvc_audio_plan_segments")
        tiles = np.zeros((n_tiles.value, 4), dtype=np.int32)
        check(L.mcvc_audio_plan_segments(st.ctypes.data, ln.ctypes.data, n, frame_offs.ctypes.data, tiles.ctypes.data, n_tiles.value, ctypes.byref(n_tiles)),
              "mcvc_audio_plan_segments")
        total = int(frame_offs[-1])
        with torch.cuda.device(self.device):
            tiles_d = torch.from_numpy(tiles).to(self.device)
            out = torch.empty(N_MEL, total, dtype=torch.float32, device=self.device)
            check(L.mcvc_audio_log_mel(ptr(wave), int(wave.numel()), ptr(tiles_d), tiles.shape[0], ptr(self.basis()), ptr(out), total, stream()),
                  "mcvc_audio_log_mel")
        return out, frame_offs

    def _detector(self):
        from data_preprocessing.silence import SilenceDetector
        if getattr(self, "_silence", None) is None:
            self._silence = SilenceDetector(self.device)
        return self._silence

    def _bank_trimmed(self, wave, lengths, trim_db, return_bounds):
        """The 22050 Hz device bank ``wave`` -> mels of every utterance between its first and last non-silent frame
        (data_preprocessing/silence.py), from the one log-mel launch over the trimmed segments in place."""
        bounds = self._detector().trim(wave, trim_db, lengths=lengths)
        offs = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])
        out, fo = self._launch_segments(wave, [int(offs[i]) + s for i, (s, _) in enumerate(bounds)], [e - s for s, e in bounds])
        host = out.cpu().numpy()
        mels = [np.ascontiguousarray(host[:, fo[i]:fo[i + 1]]) for i in range(len(lengths))]
        return (mels, bounds) if return_bounds else mels

    def _device_bank(self, waveforms, rates=None):
        """-> (contiguous float32 device bank at 22050 Hz, lengths): an upload, or ``bank_at_rates``' resampling."""
        import torch
        if rates is not None:
            return self._resampled_bank(waveforms, rates)
        ws = [np.ascontiguousarray(w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w, dtype=np.float32).reshape(-1) for w in waveforms]
        return torch.from_numpy(np.concatenate(ws)).to(self.device), [w.size for w in ws]

    def bank(self, waveforms, trim_db=None, return_bounds=False):
        """list of 1-D waveforms (numpy or tensors, any float type) -> list of float32 numpy [80, T_i], from a single launch.
        ``trim_db`` (default None: off): every utterance is trimmed to its first .. last frame within ``trim_db`` dB of its loudest one
        (data_preprocessing/silence.py; detection and mels from the one uploaded bank); ``return_bounds``: -> (mels, [(start, end)])."""
        import torch
        if trim_db is not None:
            from data_preprocessing.silence import threshold_ratio
            threshold_ratio(trim_db)
            if not len(waveforms):
                return ([], []) if return_bounds else []
            wave, lengths = self._device_bank(waveforms)
            for k in lengths:
                num_frames(k)
            return self._bank_trimmed(wave, lengths, trim_db, return_bounds)
        ws = [np.ascontiguousarray(w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w, dtype=np.float32).reshape(-1) for w in waveforms]
        if not ws:
            return []
        lengths = [w.size for w in ws]
        for k in lengths:
            num_frames(k)
        wave = torch.from_numpy(np.concatenate(ws)).to(self.device)
        out, fo = self._launch(wave, lengths)
        host = out.cpu().numpy()
        return [np.ascontiguousarray(host[:, fo[i]:fo[i + 1]]) for i in range(len(ws))]

    def bank_split(self, waveforms, top_db, min_silence_ms=300.0, rates=None, return_segments=False):
        """Long recordings -> one mel per kept interval of ``SilenceDetector.split`` (non-silent runs, merged over gaps under
        ``min_silence_ms``, intervals under 16384 samples dropped), in file order and then time order; ``rates``: as ``bank_at_rates``.
        ``return_segments``: -> (mels, [(start, end)] in samples of the 22050 Hz file, index of the file of each utterance,
        {"dropped": intervals dropped per file, "samples": 22050 Hz samples per file})."""
        from data_preprocessing.silence import gap_samples, threshold_ratio
        threshold_ratio(top_db)
        gap_samples(min_silence_ms)
        if rates is not None and len(waveforms) != len(rates):
            raise ValueError("%d waveforms but %d rates" % (len(waveforms), len(rates)))
        if not len(waveforms):
            return ([], [], [], {"dropped": [], "samples": []}) if return_segments else []
        wave, lengths = self._device_bank(waveforms, rates)
        kept, dropped = self._detector().split(wave, top_db, min_silence_ms, lengths=lengths, return_dropped=True)
        offs = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])
        intervals = [iv for per_file in kept for iv in per_file]
        index = [i for i, per_file in enumerate(kept) for _ in per_file]
        mels = []
        if intervals:
            out, fo = self._launch_segments(wave, [int(offs[i]) + s for i, (s, _) in zip(index, intervals)], [e - s for s, e in intervals])
            host = out.cpu().numpy()
            mels = [np.ascontiguousarray(host[:, fo[i]:fo[i + 1]]) for i in range(len(intervals))]
        return (mels, intervals, index, {"dropped": dropped, "samples": [int(k) for k in lengths]}) if return_segments else mels

    def _resampled_bank(self, waveforms, rates):
        """``bank_at_rates``' first half: -> (contiguous float32 device bank at 22050 Hz in the caller's order, lengths)."""
        import torch
        from data_preprocessing.resample import Resampler
        if getattr(self, "_resampler", None) is None:
            self._resampler = Resampler(self.device)
        groups = {}
        for i, r in enumerate(rates):
            groups.setdefault(int(r), []).append(i)
        parts = [None] * len(waveforms)
        for r, idx in groups.items():
            dev, offs = self._resampler.bank([waveforms[i] for i in idx], r, SAMPLING_RATE)
            for k, i in enumerate(idx):
                parts[i] = dev[int(offs[k]):int(offs[k + 1])]
        lengths = [int(p.numel()) for p in parts]
        return (torch.cat(parts) if len(parts) > 1 else parts[0].contiguous()), lengths

    def bank_at_rates(self, waveforms, rates, trim_db=None, return_bounds=False):
        """``bank`` for utterances recorded at different rates: waveform i is at ``rates[i]`` Hz.  Each group of equal rate is resampled
        to 22050 Hz on the device (one launch per distinct rate, data_preprocessing/resample.py), the 22050 Hz bank is assembled on the
        device in the caller's order and goes through the one log-mel launch; no waveform returns to the host in between.
        ``trim_db`` / ``return_bounds``: as ``bank``; silence is detected on the 22050 Hz bank, after resampling, and the bounds are in its
        samples."""
        if len(waveforms) != len(rates):
            raise ValueError("%d waveforms but %d rates" % (len(waveforms), len(rates)))
        if trim_db is not None:
            from data_preprocessing.silence import threshold_ratio
            threshold_ratio(trim_db)
        if not len(waveforms):
            return ([], []) if trim_db is not None and return_bounds else []
        wave, lengths = self._resampled_bank(waveforms, rates)
        for k in lengths:
            num_frames(k)
        if trim_db is not None:
            return self._bank_trimmed(wave, lengths, trim_db, return_bounds)
        out, fo = self._launch(wave, lengths)
        host = out.cpu().numpy()
        return [np.ascontiguousarray(host[:, fo[i]:fo[i + 1]]) for i in range(len(lengths))]

    def __call__(self, x):
        import torch
        from mask_cyclegan_vc._hip import require_on_device
        require_on_device("data_preprocessing.audio2mel", x, self.device, "waveform", "front-end")
        if x.dim() == 3 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 2:
            raise ValueError("expected a [B, 1, L] or [B, L] waveform tensor, got %s" % (tuple(x.shape),))
        B, n = x.shape
        T = num_frames(n)
        wave = x.to(torch.float32).contiguous()
        out, _ = self._launch(wave, [n] * B)
        return out.view(N_MEL, B, T).permute(1, 0, 2).contiguous()
