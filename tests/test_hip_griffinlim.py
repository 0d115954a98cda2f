"""GPU: the Griffin-Lim decoder (csrc/griffinlim_kernels.hip via mask_cyclegan_vc.griffinlim.GriffinLimVocoder) and the
``--griffin_lim`` path of the inference driver.

The checker is griffinlim_checker.py: the transform restated with torch.stft / irfft and an explicit overlap-add on the CPU -- float64
is the truth, float32 the yardstick.  Distances are the whole-tensor rel-L2 and the max abs error over the peak of the truth.  The
kernel passes at max(2e-6, k x the float32 checker's own distance to float64 at the same input): k = 2 one transform deep (n_iter 0
or 1, mel inversion alone), k = 4 for longer chains (the matrix-product DFT sums 1024 terms in another order than the FFT and the
iteration carries that forward).  The floor comes from CPU measurements of the float32 checker (2.4e-7 .. 7.4e-7 after one iteration),
not from the kernel.  Every test prints its figures before it asserts."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch
from scipy.io import wavfile

pytestmark = pytest.mark.gpu

import audio_checker as ack  # noqa: E402
import griffinlim_checker as ck  # noqa: E402
import mcvc_oracle as orc  # noqa: E402  (filler parameters only)
from data_preprocessing.audio2mel import Audio2Mel, read_wav  # noqa: E402
from mask_cyclegan_vc import _hip  # noqa: E402
from mask_cyclegan_vc.griffinlim import ZERO_PHASE, GriffinLimVocoder  # noqa: E402

MCVC_ERR_INVALID, MCVC_ERR_WORKSPACE = 1001, 1002
EDGE_T = [2, 3, 4, 7]                                       # every frame touches a reflected edge; T = 2 reflects at both ends of a frame
TILE_T = [61, 63, 64, 65, 67]                               # around a 64-frame tile and its 3-frame overlap
ALL_T = EDGE_T + TILE_T + [129]
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def gl():
    return GriffinLimVocoder()


@pytest.fixture(scope="module")
def recording(golden_dir):
    return read_wav(os.path.join(golden_dir, "audio", "real_VCC2SF3.wav"))


@pytest.fixture(scope="module")
def speech_mel(recording):
    """float64 [80, 224] log-mel of the committed recording, by the front-end's checker."""
    return ack.log_mel(recording).numpy()


@pytest.fixture(scope="module")
def noise_mel():
    return ack.log_mel(0.1 * np.random.RandomState(11).randn(256 * 8 + 300)).numpy()[:, :8]


def random_angles(B, T, seed):
    th = 2.0 * np.pi * np.random.RandomState(seed).rand(B, 513, T)
    return np.stack([np.cos(th), np.sin(th)], axis=-1).astype(np.float32)


def mel_batch(mel, T, B, start=20):
    """B windows of T frames of a [80, .] log-mel as float32, each with its own offset: neighbours differ at the joints."""
    return np.stack([mel[:, start + 5 * b:start + 5 * b + T] + 0.1 * b for b in range(B)]).astype(np.float32)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def both_checkers(x, kind, angles, n_iter, momentum):
    """(truth, the float32 checker's result, the float64 magnitude) for the float32 input ``x`` the kernel gets."""
    if kind == "mel":
        M64, M32 = ck.magnitude_from_mel(x, F64), ck.magnitude_from_mel(x, F32)
    else:
        M64, M32 = torch.from_numpy(x).to(F64), torch.from_numpy(x).to(F32)
    return ck.griffin_lim(M64, angles, n_iter, momentum, F64), ck.griffin_lim(M32, angles, n_iter, momentum, F32), M64


def run(gl, x, kind, angles, n_iter, momentum):
    fn = gl.inverse if kind == "mel" else gl.from_magnitude
    got = fn(dev(x), angles=ZERO_PHASE if angles is None else dev(angles), n_iter=n_iter, momentum=momentum)
    B, T = x.shape[0], x.shape[2]
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (B, 256 * T) and got.is_contiguous() and not got.requires_grad
    return got.cpu().numpy()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", ALL_T)
def test_1_istft_alone(gl, T, B):
    """n_iter = 0 on a linear input: random magnitude times random angles, the imaginary parts of bins 0 and 512 included (no effect)."""
    rs = np.random.RandomState(1000 + 10 * T + B)
    mag = (rs.rand(B, 513, T) + 0.5 * np.arange(B)[:, None, None]).astype(np.float32)
    ang = random_angles(B, T, 2000 + T)
    assert np.abs(ang[:, 0, :, 1]).min() > 0 and np.abs(ang[:, 512, :, 1]).min() > 0
    got = run(gl, mag, "lin", ang, 0, 0.99)
    truth, ref32, _ = both_checkers(mag, "lin", ang, 0, 0.99)
    ck.check("1 ISTFT alone B=%d T=%d" % (B, T), got, truth, ref32, 2)
    real = ang.copy()
    real[:, (0, 512), :, 1] = 0.0                            # the same call without those imaginary parts: the same bits
    assert np.array_equal(run(gl, mag, "lin", real, 0, 0.99), got)


@pytest.mark.parametrize("T", [7, 67, 129])
def test_2_round_trip_of_a_recording(gl, recording, T):
    """from_magnitude(|STFT(x)|, angles = phase of STFT(x), n_iter = 0) gives back x; the STFT comes from the float64 checker."""
    x = recording[4000:4000 + 256 * T].astype(np.float64)[None]
    S = ck.stft(x)
    mag = S.abs().numpy().astype(np.float32)
    ph = (S / S.abs().clamp(min=1e-300)).numpy()
    ang = np.stack([ph.real, ph.imag], axis=-1).astype(np.float32)
    got = run(gl, mag, "lin", ang, 0, 0.0)
    ref32 = ck.griffin_lim(torch.from_numpy(mag), ang, 0, 0.0, F32)       # the float32 checker on the same float32 inputs
    ck.check("2 round trip T=%d" % T, got, torch.from_numpy(x), ref32, 2)


@pytest.mark.parametrize("kind", ["mel", "lin"])
@pytest.mark.parametrize("T", ALL_T)
def test_3_one_iteration(gl, speech_mel, T, kind):
    """One forward-plus-update step, with momentum 0 and 0.99 (R_-1 = 0: the stored R must not be read on the first step)."""
    B = 3
    if kind == "mel":
        x = mel_batch(speech_mel, T, B)
    else:
        x = (np.random.RandomState(3000 + T).rand(B, 513, T) * (1.0 + np.arange(B)[:, None, None])).astype(np.float32)
    ang = random_angles(B, T, 3100 + T)
    for momentum in (0.0, 0.99):
        got = run(gl, x, kind, ang, 1, momentum)
        truth, ref32, _ = both_checkers(x, kind, ang, 1, momentum)
        ck.check("3 one iteration %s B=%d T=%d m=%.2f" % (kind, B, T, momentum), got, truth, ref32, 2)


@pytest.mark.parametrize("T", [8, 67])
def test_4_mel_inversion_alone(gl, speech_mel, noise_mel, T):
    """n_iter = 0, zero phase, mel input, against the checker's ISTFT of the float64 magnitude: speech (its pinv product goes negative
    and is clipped), a mel on the front-end's clamp (-5.0 everywhere), and noise."""
    speech = mel_batch(speech_mel, T, 1)[0]
    clamp = np.full((80, T), -5.0, dtype=np.float32)
    noisy = np.tile(noise_mel, (1, (T + 7) // 8))[:, :T].astype(np.float32) + 0.2
    x = np.stack([speech, clamp, noisy])
    raw = torch.from_numpy(ck.pinv_basis()) @ (10.0 ** torch.from_numpy(x[0]).double())
    clipped = float((raw < 0).double().mean())
    print("4 mel inversion T=%d: %.2f %% of the speech magnitude entries are clipped at 0" % (T, 100 * clipped))
    assert clipped > 0
    got = run(gl, x, "mel", None, 0, 0.99)
    truth, ref32, M64 = both_checkers(x, "mel", None, 0, 0.99)
    assert float((truth - ck.istft(M64.to(torch.complex128))).abs().max()) == 0.0
    for b, name in enumerate(("speech", "clamp", "noise")):
        ck.check("4 mel inversion %s T=%d" % (name, T), got[b:b + 1], truth[b:b + 1], ref32[b:b + 1], 2)
    ck.check("4 mel inversion batch T=%d" % T, got, truth, ref32, 2)


@pytest.mark.parametrize("momentum", [0.0, 0.99])
@pytest.mark.parametrize("n_iter", [4, 32])
@pytest.mark.parametrize("case", ["speech8", "speech67", "noise8"])
def test_5_chains(gl, speech_mel, noise_mel, case, n_iter, momentum):
    """Longer chains from the module's own seeded angles: the waveform gate (k = 4) and the spectral convergence
    || |STFT(x)| - M || / || M || of the kernel's output, evaluated in float64, within 1 % of the float64 run's."""
    T = 67 if case == "speech67" else 8
    x = (noise_mel[None] if case == "noise8" else mel_batch(speech_mel, T, 1)).astype(np.float32)
    ang = gl.angles(1, T).cpu().numpy()
    got = gl.inverse(dev(x), n_iter=n_iter, momentum=momentum).cpu().numpy()
    assert np.array_equal(got, run(gl, x, "mel", ang, n_iter, momentum))      # the default angles ARE the seeded draw
    truth, ref32, M64 = both_checkers(x, "mel", ang, n_iter, momentum)
    sc_got, sc_truth, sc_32 = ck.spectral_convergence(got, M64), ck.spectral_convergence(truth, M64), ck.spectral_convergence(ref32, M64)
    print("5 chain %s n_iter=%d m=%.2f: spectral convergence kernel %.5f  float64 %.5f  float32 checker %.5f  (kernel / float64 - 1 = %+.2e)"
          % (case, n_iter, momentum, sc_got, sc_truth, sc_32, sc_got / sc_truth - 1))
    ck.check("5 chain %s n_iter=%d m=%.2f" % (case, n_iter, momentum), got, truth, ref32, 4)
    assert abs(sc_got - sc_truth) <= 0.01 * sc_truth


def test_6_batches_seeds_and_bits(gl, speech_mel):
    T = 65
    x = dev(mel_batch(speech_mel, T, 3))
    whole = gl.inverse(x, n_iter=4)
    for b in range(3):
        assert torch.equal(gl.inverse(x[b:b + 1], n_iter=4)[0], whole[b]), b
    assert torch.equal(gl.inverse(x, n_iter=4), whole)
    assert torch.equal(GriffinLimVocoder(seed=0).inverse(x, n_iter=4), whole)
    other = GriffinLimVocoder(seed=1).inverse(x, n_iter=4)
    assert not torch.equal(other, whole) and float((other - whole).abs().max()) > 1e-3 * float(whole.abs().max())
    assert torch.equal(gl.angles(3, T)[2], gl.angles(1, T)[0])
    mag = dev(np.random.RandomState(6).rand(2, 513, 5).astype(np.float32))
    assert torch.equal(gl.from_magnitude(mag, n_iter=2), gl.from_magnitude(mag, n_iter=2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        gl.inverse(x.cpu())
    with pytest.raises(ValueError, match="at least 2 frames"):
        gl.inverse(x[:, :, :1])
    with pytest.raises(ValueError, match="negative"):
        gl.from_magnitude(-mag)
    wave = dev(0.1 * np.random.RandomState(7).randn(2, 5000).astype(np.float32))
    assert torch.equal(gl(wave), Audio2Mel()(wave))           # __call__ is the front-end


def test_7_bad_arguments_are_refused_and_write_nothing(gl, speech_mel):
    L = _hip.lib()
    B, T = 2, 5
    x = dev(mel_batch(speech_mel, T, B))
    ang = gl.angles(B, T)
    tables = gl.tables()
    n = L.mcvc_gl_workspace_floats(B, T)
    ws = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
    out = torch.full((B, 256 * T + 4), 7.0, device="cuda")
    p, s = _hip.ptr, _hip.stream()
    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    good = [p(x), 0, p(ang), p(tables), p(out), p(ws), n, B, T, 2, 0.99, s]
    for k, bad, code in ((0, None, MCVC_ERR_INVALID), (3, None, MCVC_ERR_INVALID), (4, None, MCVC_ERR_INVALID),     # null in / tables / out
                         (5, None, MCVC_ERR_WORKSPACE),                                                             # null workspace
                         (0, off(x, 2), MCVC_ERR_INVALID), (2, off(ang, 4), MCVC_ERR_INVALID), (3, off(tables, 4), MCVC_ERR_INVALID),
                         (4, off(out, 1), MCVC_ERR_INVALID), (5, off(ws, 4), MCVC_ERR_INVALID),                     # misaligned
                         (8, 1, MCVC_ERR_INVALID), (7, 0, MCVC_ERR_INVALID), (9, -1, MCVC_ERR_INVALID), (1, 2, MCVC_ERR_INVALID),
                         (10, 1.0, MCVC_ERR_INVALID), (10, -0.5, MCVC_ERR_INVALID), (6, n - 1, MCVC_ERR_WORKSPACE)):
        args = list(good)
        args[k] = bad
        assert L.mcvc_gl_decode(*args) == code, (k, bad)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0.0).all())
    assert L.mcvc_gl_decode(*good) == 0                                  # and the untouched arguments do work
    torch.cuda.synchronize()
    assert torch.equal(out.view(-1)[:B * 256 * T].view(B, 256 * T), gl.inverse(x, n_iter=2, momentum=0.99))
    assert bool((out.view(-1)[B * 256 * T:] == 7.0).all()) and bool((ws[n:] == 0.0).all())


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)))


def test_8_inference_cli(tmp_path, golden_dir):
    """python -m mask_cyclegan_vc.test --griffin_lim 8 --wav_dir <the two committed recordings>: the reference's four file names, float32
    at 22050 Hz with 256 T samples; the original's wav, sent through the front-end again, is as close to the de-normalised source mel
    (RMS in log10 units) as the float64 checker's own wav -> mel -> GL(8) -> mel on the same recording, times 1.25."""
    from mask_cyclegan_vc import test as test_cli
    clips = os.path.join(golden_dir, "audio")
    names = sorted(n for n in os.listdir(clips) if n.endswith(".wav"))
    assert names == ["real_VCC2SF3.wav", "real_VCC2TF1.wav"]
    waves = [read_wav(os.path.join(clips, n)) for n in names]
    data = str(tmp_path / "data")
    rs = np.random.RandomState(4)
    stat = {}
    for spk in ("SPKA", "SPKB"):
        os.makedirs(os.path.join(data, spk))
        with open(os.path.join(data, spk, "%s_normalized.pickle" % spk), "wb") as fh:
            pickle.dump([rs.randn(80, 64).astype(np.float32)], fh)
        stat[spk] = dict(mean=(-2.0 + rs.randn(80, 1)).astype(np.float32), std=(1 + rs.rand(80, 1)).astype(np.float32))
        np.savez(os.path.join(data, spk, "%s_norm_stat.npz" % spk), **stat[spk])
    ck_dir = tmp_path / "ckpts"
    ck_dir.mkdir()
    torch.save({"ckpt_info": {"epoch": 1}, "model_class": "Generator", "model_state": orc.filler_params("G", 11), "optimizer": None,
                "lr_scheduler": None}, str(ck_dir / "00001_generator_A2B.pth.tar"))
    common = ["--save_dir", str(tmp_path / "res"), "--preprocessed_data_dir", data, "--speaker_A_id", "SPKA", "--speaker_B_id", "SPKB",
              "--ckpt_dir", str(ck_dir), "--load_epoch", "1", "--model_name", "generator_A2B", "--wav_dir", clips]
    test_cli.main(["--name", "without"] + common)
    assert sorted(os.listdir(str(tmp_path / "res" / "without"))) == ["converted_mel", "test_args.json"]      # no converted_audio/
    test_cli.main(["--name", "with", "--griffin_lim", "8"] + common)
    out = str(tmp_path / "res" / "with" / "converted_audio")
    assert sorted(os.listdir(out)) == sorted("%d-%s_SPKA_to_SPKB.wav" % (i, k) for i in (0, 1) for k in ("converted", "original"))
    for i in (0, 1):
        assert np.array_equal(np.load(str(tmp_path / "res" / "with" / "converted_mel" / ("%d-converted_SPKA_to_SPKB.npy" % i))),
                              np.load(str(tmp_path / "res" / "without" / "converted_mel" / ("%d-converted_SPKA_to_SPKB.npy" % i))))
    fft, gl = Audio2Mel(), GriffinLimVocoder(n_iter=8)
    for i, (w, T) in enumerate(zip(waves, (224, 225))):
        for k in ("converted", "original"):
            rate, wav = wavfile.read(os.path.join(out, "%d-%s_SPKA_to_SPKB.wav" % (i, k)))
            frames = T if k == "original" else np.load(str(tmp_path / "res" / "with" / "converted_mel" / ("%d-converted_SPKA_to_SPKB.npy" % i))).shape[1]
            assert frames >= T                                # (the generator rounds its time axis up)
            assert rate == 22050 and wav.dtype == np.float32 and wav.shape == (256 * frames,) and np.isfinite(wav).all() and np.abs(wav).max() > 0
        # what the driver decoded: the front-end's mel, standardised with speaker A's statistics and de-normalised again, in float32
        (mel,) = fft.bank([w])
        src = (((mel - stat["SPKA"]["mean"]) / stat["SPKA"]["std"]).astype(np.float32) * stat["SPKA"]["std"] + stat["SPKA"]["mean"]).astype(np.float32)
        assert np.array_equal(wav, gl.inverse(dev(src[None]))[0].cpu().numpy())          # the file is the module's decode of that mel
        (again,) = fft.bank([wav])
        d = _rms(again, src)
        mel64 = ack.log_mel(w)
        ang = gl.angles(1, T).cpu().numpy()
        wav64 = ck.griffin_lim(ck.magnitude_from_mel(mel64[None]), ang, 8, 0.99, F64)[0]
        d64 = _rms(ack.log_mel(wav64.numpy()), mel64)
        print("8 CLI utterance %d T=%d: log-mel RMS distance after wav -> mel: driver %.4f, float64 checker %.4f (ratio %.3f, gate 1.25)"
              % (i, T, d, d64, d / d64))
        assert d <= 1.25 * d64
