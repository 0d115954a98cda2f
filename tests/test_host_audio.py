"""CPU-only checks of the wav -> log-mel front-end's host side (data_preprocessing/audio2mel.py, the mcvc_audio_* C ABI): the Slaney
mel basis against the values pinned by its definition, the frame-count law, .wav reading, the preprocessing CLI's flags.  No kernel
is launched here."""
import ctypes

import numpy as np
import pytest
from scipy.io import wavfile

import audio_checker as ck
from data_preprocessing import audio2mel, preprocess_vcc2018
from mask_cyclegan_vc import _hip

MCVC_ERR_INVALID, MCVC_ERR_WORKSPACE = 1001, 1002
FRAME_LAW = {385: 1, 511: 1, 512: 2, 1023: 3, 1024: 4, 1025: 4, 57344: 224}      # T = (L - 256) // 256 + 1


def test_mel_basis_matches_its_definition():
    B = audio2mel.mel_filterbank(np.float64)
    assert B.shape == (80, 513)
    assert abs(B.sum() - 3.7146471721) < 1e-9 and abs(B.max() - 0.0241469011) < 1e-9
    assert (B >= 0).all() and (B.sum(axis=1) > 0).all()                          # no empty row
    np.testing.assert_allclose(B[0, :4], [0, 0.01276074, 0.02316559, 0.01040485], atol=5e-9)
    np.testing.assert_allclose(B[79, -4:], [3.1545e-4, 2.1030e-4, 1.0515e-4, 0], atol=5e-9)
    assert ((B > 0).sum(axis=0) <= 2).all()                                      # each bin feeds at most two filters
    np.testing.assert_allclose(B, ck.slaney_mel_basis(), rtol=0, atol=1e-15)     # the checker's scalar restatement
    B32 = audio2mel.mel_filterbank()
    assert B32.dtype == np.float32 and np.array_equal(B32, B.astype(np.float32))


def test_library_mel_table_is_the_same_basis():
    """The sparse table behind the DFT basis in the kernel's constant operand, expanded: the float32 basis, bit for bit."""
    L = _hip.lib()
    n = L.mcvc_audio_basis_floats()
    assert n > 1024 * 1024
    host = np.full(n, np.nan, dtype=np.float32)
    assert L.mcvc_audio_basis_init(host.ctypes.data) == 0
    assert L.mcvc_audio_basis_init(None) == MCVC_ERR_INVALID
    assert np.isfinite(host[:1024 * 1024]).all() and np.abs(host[:1024 * 1024]).max() <= 1.0
    head, wts = host[1024 * 1024:1024 * 1024 + 256].view(np.int32), host[1024 * 1024 + 256:]
    B = np.zeros((80, 513), dtype=np.float32)
    for i in range(80):
        lo, cnt, off = head[i], head[80 + i], head[160 + i]
        B[i, lo:lo + cnt] = wts[off:off + cnt]
    assert np.array_equal(B, audio2mel.mel_filterbank())


def test_forward_basis_fill_against_numpy():
    """W[row][k], the lane order undone: rows 2b / 2b + 1 = hann[k] cos / sin(2 pi k b / 1024) of bin b = 1..511, row 0 the window itself
    (bin 0) and row 1 the Nyquist cosine hann[k] (-1)^k -- the sines of bins 0 and 512 are zero and have no row."""
    L = _hip.lib()
    N = 1024
    host = np.empty(L.mcvc_audio_basis_floats(), dtype=np.float32)
    assert L.mcvc_audio_basis_init(host.ctypes.data) == 0
    # float index ((mt * 128 + kg) * 64 + 32 half + l31) * 4 + j  ->  W[row 32 mt + l31][k = 8 kg + 2 j + half]
    W = host[:N * N].reshape(32, 128, 2, 32, 4).transpose(0, 3, 1, 4, 2).reshape(N, N).astype(np.float64)
    k = np.arange(N)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * k / N)
    want = np.zeros((N, N))
    want[0] = w
    want[1] = w * np.where(k % 2 == 0, 1.0, -1.0)
    for b in range(1, 512):
        ph = 2.0 * np.pi * ((k * b) % N) / N                   # exact argument reduction
        want[2 * b] = w * np.cos(ph)
        want[2 * b + 1] = w * np.sin(ph)
    err = float(np.abs(W - want).max())
    print("forward basis: max abs difference %.3e (one float32 ulp of the largest entry: %.3e)" % (err, 2.0 ** -23))
    assert err <= 2.0 ** -23                                    # the inverse fill's rule: float32 rounding of values up to 1, cos / sin of two libraries
    # as an operator: the basis applied to a frame gives the packed rfft of the windowed frame, (Re, -Im) per bin
    x = np.random.RandomState(0).randn(N)
    S = np.fft.rfft(w * x)
    packed = np.zeros(N)
    packed[0], packed[1], packed[2::2], packed[3::2] = S[0].real, S[512].real, S[1:512].real, -S[1:512].imag
    assert np.abs(W @ x - packed).max() <= 2.0 ** -23 * np.abs(x).sum()      # every basis entry within one float32 ulp of 1


def test_frame_count_law():
    L = _hip.lib()
    for n in (0, 1, 384):
        assert L.mcvc_audio_frames(n) == 0
        with pytest.raises(ValueError, match="at least 385 samples"):
            audio2mel.num_frames(n)
    with pytest.raises(RuntimeError):                                            # torch refuses L = 384 too
        ck.log_mel(np.zeros(384))
    for n, T in FRAME_LAW.items():
        assert L.mcvc_audio_frames(n) == T == audio2mel.num_frames(n), n
    for n in (385, 511, 512, 1023, 1024, 1025):
        assert ck.log_mel(np.zeros(n)).shape == (80, FRAME_LAW[n])


def test_plan_lists_every_frame_once_and_refuses_short_utterances():
    L = _hip.lib()
    lens = [385, 57344, 16384, 16640, 512]                                       # 1, 224, 64, 65 and 2 frames
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    fo = np.zeros(len(lens) + 1, dtype=np.int32)
    nt = ctypes.c_int(-1)
    assert L.mcvc_audio_plan(offs.ctypes.data, len(lens), fo.ctypes.data, None, 0, ctypes.byref(nt)) == 0
    frames = [FRAME_LAW.get(n, (n - 256) // 256 + 1) for n in lens]
    assert fo.tolist() == np.concatenate([[0], np.cumsum(frames)]).tolist() and nt.value == 1 + 4 + 1 + 2 + 1
    tiles = np.zeros((nt.value, 4), dtype=np.int32)
    assert L.mcvc_audio_plan(offs.ctypes.data, len(lens), fo.ctypes.data, tiles.ctypes.data, nt.value - 1, ctypes.byref(nt)) == MCVC_ERR_WORKSPACE
    assert L.mcvc_audio_plan(offs.ctypes.data, len(lens), fo.ctypes.data, tiles.ctypes.data, nt.value, ctypes.byref(nt)) == 0
    covered = []
    for s0, n, col0, t0 in tiles.tolist():
        u = offs.tolist().index(s0)
        assert n == lens[u] and col0 == fo[u] + t0 and t0 % 64 == 0
        covered += list(range(col0, fo[u] + min(frames[u], t0 + 64)))
    assert covered == list(range(sum(frames)))
    bad = np.array([0, 1000, 1384, 3000], dtype=np.int32)                        # the middle utterance has 384 samples
    assert L.mcvc_audio_plan(bad.ctypes.data, 3, fo.ctypes.data, None, 0, ctypes.byref(nt)) == MCVC_ERR_INVALID
    assert L.mcvc_audio_plan(offs.ctypes.data, 0, fo.ctypes.data, None, 0, ctypes.byref(nt)) == MCVC_ERR_INVALID
    assert L.mcvc_audio_plan(None, 1, fo.ctypes.data, None, 0, ctypes.byref(nt)) == MCVC_ERR_INVALID


def _tone(n, rate, f=440.0, seed=0):
    t = np.arange(n) / rate
    return 0.4 * np.sin(2 * np.pi * f * t) + 0.05 * np.random.RandomState(seed).randn(n)


def test_read_wav_int16_mono(tmp_path):
    pcm = (_tone(3000, 22050) * 32767).astype(np.int16)
    pcm[:2] = [-32768, 32767]
    wavfile.write(str(tmp_path / "a.wav"), 22050, pcm)
    x = audio2mel.read_wav(tmp_path / "a.wav")
    assert x.dtype == np.float32 and x.shape == (3000,)
    assert np.array_equal(x, pcm.astype(np.float32) / 32768.0) and x[0] == -1.0


def test_read_wav_int16_stereo_is_the_channel_mean(tmp_path):
    pcm = np.stack([(_tone(3000, 22050, 440, 1) * 32767).astype(np.int16), (_tone(3000, 22050, 660, 2) * 32767).astype(np.int16)], axis=1)
    wavfile.write(str(tmp_path / "s.wav"), 22050, pcm)
    x = audio2mel.read_wav(tmp_path / "s.wav")
    assert x.dtype == np.float32 and x.shape == (3000,)
    want = (pcm.astype(np.float64) / 32768.0).mean(axis=1)
    np.testing.assert_allclose(x, want, rtol=0, atol=2.0 ** -24)


def test_read_wav_float32(tmp_path):
    w = _tone(3000, 22050).astype(np.float32)
    wavfile.write(str(tmp_path / "f.wav"), 22050, w)
    x = audio2mel.read_wav(tmp_path / "f.wav")
    assert x.dtype == np.float32 and np.array_equal(x, w)


def test_read_wav_16khz_is_resampled_to_22050(tmp_path):
    from scipy.signal import resample_poly
    pcm = (_tone(16000, 16000) * 32767).astype(np.int16)
    wavfile.write(str(tmp_path / "r.wav"), 16000, pcm)
    x = audio2mel.read_wav(tmp_path / "r.wav")
    assert x.dtype == np.float32 and x.shape == (22050,)
    np.testing.assert_allclose(x, resample_poly(pcm.astype(np.float64) / 32768.0, 441, 320), rtol=0, atol=1e-6)
    spec = np.abs(np.fft.rfft(x))                                                # one second: bin = Hz
    assert int(spec.argmax()) == 440


def test_read_wav_refuses_what_is_not_pcm(tmp_path):
    p = tmp_path / "junk.wav"
    p.write_bytes(b"this is not a RIFF file at all" * 10)
    with pytest.raises(ValueError, match="not a readable"):
        audio2mel.read_wav(p)
    with pytest.raises(FileNotFoundError):
        audio2mel.read_wav(tmp_path / "missing.wav")


def test_wave_module_fallback_reads_the_same_samples(tmp_path):
    pcm = np.stack([(_tone(2000, 22050, 440, 3) * 32767).astype(np.int16), (_tone(2000, 22050, 550, 4) * 32767).astype(np.int16)], axis=1)
    wavfile.write(str(tmp_path / "s.wav"), 22050, pcm)
    rate, data = audio2mel._read_with_wave_module(str(tmp_path / "s.wav"))
    assert rate == 22050 and np.array_equal(data, pcm)
    wavfile.write(str(tmp_path / "f.wav"), 22050, _tone(2000, 22050).astype(np.float32))     # IEEE float: not PCM for the stdlib
    with pytest.raises(ValueError, match="not a readable"):
        audio2mel._read_with_wave_module(str(tmp_path / "f.wav"))


def test_fixture_recordings_have_the_documented_lengths(golden_dir):
    for name, n, T in (("real_VCC2SF3.wav", 57344, 224), ("real_VCC2TF1.wav", 57600, 225)):
        x = audio2mel.read_wav("%s/audio/%s" % (golden_dir, name))
        assert x.shape == (n,) and audio2mel.num_frames(n) == T and 0.05 < np.abs(x).max() <= 1.0


def test_preprocess_parser_wants_exactly_one_input_directory(tmp_path, capsys):
    common = ["--preprocessed_data_directory", str(tmp_path / "out"), "--speaker_ids", "A"]
    with pytest.raises(SystemExit):
        preprocess_vcc2018.main(["--data_directory", "w", "--mel_directory", "m"] + common)
    assert "not allowed with" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        preprocess_vcc2018.main(common)
    assert "one of the arguments" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()
    a = preprocess_vcc2018.build_parser().parse_args(["--data_directory", "w"] + common)
    assert a.data_directory == "w" and a.mel_directory is None
    a = preprocess_vcc2018.build_parser().parse_args(["--mel_directory", "m"] + common)
    assert a.mel_directory == "m" and a.data_directory is None


def test_mel_directory_path_behaves_as_before(tmp_path):
    import pickle
    rs = np.random.RandomState(0)
    mels = [rs.randn(80, T).astype(np.float32) for T in (70, 63, 100)]
    (tmp_path / "m" / "A").mkdir(parents=True)
    for i, m in enumerate(mels):
        np.save(str(tmp_path / "m" / "A" / ("%d.npy" % i)), m)
    preprocess_vcc2018.main(["--mel_directory", str(tmp_path / "m"), "--preprocessed_data_directory", str(tmp_path / "out"), "--speaker_ids", "A"])
    want, mean, std = preprocess_vcc2018.normalize_mels(mels)
    with open(str(tmp_path / "out" / "A" / "A_normalized.pickle"), "rb") as fh:
        got = pickle.load(fh)
    assert len(got) == 2 and all(np.array_equal(g, w) for g, w in zip(got, want))
    stat = np.load(str(tmp_path / "out" / "A" / "A_norm_stat.npz"))
    assert np.array_equal(stat["mean"], mean) and np.array_equal(stat["std"], std)


def test_new_symbols_are_bound():
    for name in ("mcvc_audio_frames", "mcvc_audio_basis_floats", "mcvc_audio_basis_init", "mcvc_audio_plan", "mcvc_audio_log_mel"):
        assert name in _hip._SIGS and name in _hip.EXPORTED_SYMBOLS
        assert hasattr(_hip.lib(), name)


def test_front_end_has_no_cpu_path(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        audio2mel.Audio2Mel()
    with pytest.raises(RuntimeError, match="no CPU path"):
        preprocess_vcc2018.main(["--data_directory", "nowhere", "--preprocessed_data_directory", "nowhere_out", "--speaker_ids", "A"])


def test_wav_dir_flag_is_parsed(tmp_path):
    from args.cycleGAN_test_arg_parser import CycleGANTestArgParser
    base = ["--name", "x", "--save_dir", str(tmp_path)]
    assert CycleGANTestArgParser().parse_args(base).wav_dir is None
    assert CycleGANTestArgParser().parse_args(base + ["--wav_dir", "clips"]).wav_dir == "clips"
