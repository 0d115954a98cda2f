"""GPU: the fused wav -> log-mel kernel (csrc/audio_kernels.hip via data_preprocessing.audio2mel.Audio2Mel) and the two command-line
paths that start from .wav files.

The checker is audio_checker.py: the five steps of the transform with torch.stft on the CPU -- float64 is the truth, float32 is the
reference's own arithmetic.  Gates are tied to the float32 spread at the same input (the convention of test_hip_lengths.py): the
kernel may be at most twice as far from the float64 result as the float32 checker is, with floors of 1e-4 on the maximum absolute
error (log10 units) and 2e-6 on the whole-tensor rel-L2.  The floors come from CPU measurements on the reference's four recordings
(float32 FFT 2.5e-5..4.3e-5 / 3.8e-7..6.4e-7; float32 DFT by matrix product 0.9e-5..3.5e-5 / 1.9e-7..3.0e-7), not from the kernel."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch
from scipy.io import wavfile

pytestmark = pytest.mark.gpu

import audio_checker as ck  # noqa: E402
import mcvc_oracle as orc  # noqa: E402  (filler parameters only)
from data_preprocessing import preprocess_vcc2018  # noqa: E402
from data_preprocessing.audio2mel import Audio2Mel, read_wav  # noqa: E402
from mask_cyclegan_vc import _hip  # noqa: E402
from mask_cyclegan_vc.train import load_speaker  # noqa: E402

MCVC_ERR_INVALID = 1001
EDGE_LENGTHS = [385, 511, 512, 1023, 1024, 1025, 57344]
# the ragged bank: the edge lengths, 64 / 65 frames (one workgroup exactly, one frame into the next), 129 frames, lengths off the hop
BANK_LENGTHS = [385, 57344, 511, 16384, 512, 16640, 1023, 33023, 1024, 4001, 1025, 16639, 30000]


@pytest.fixture(scope="module")
def fft():
    return Audio2Mel()


@pytest.fixture(scope="module")
def recordings(golden_dir):
    return {n: read_wav(os.path.join(golden_dir, "audio", n)) for n in ("real_VCC2SF3.wav", "real_VCC2TF1.wav")}


def noise(n, amp, seed):
    return (amp * np.random.RandomState(seed).randn(n)).astype(np.float32)


def test_fixture_recordings(fft, recordings):
    for (name, x), T in zip(recordings.items(), (224, 225)):
        (got,) = fft.bank([x])
        assert got.dtype == np.float32 and got.shape == (80, T)
        ck.check(name, got, x)


@pytest.mark.parametrize("amp", [0.1, 1e-4])
def test_noise(fft, amp):
    x = noise(20001, amp, 5)
    ck.check("noise amp %g" % amp, fft.bank([x])[0], x)


def test_click_sits_exactly_on_the_clamp(fft):
    x = np.zeros(30000, dtype=np.float32)
    x[20000] = 0.5
    (got,) = fft.bank([x])
    truth = ck.check("click", got, x).numpy()
    silent = (truth == -5.0).all(axis=0)                    # frames that do not contain the click: every value is the clamp's
    assert 0.9 < silent.mean() < 1.0, silent.mean()
    assert (got[:, silent] == -5.0).all() and got.min() == -5.0 and got[:, ~silent].max() > -5.0


def test_sine_sweep(fft):
    t = np.arange(30000) / 22050.0
    x = (0.5 * np.sin(2 * np.pi * (50.0 * t + 0.5 * (10000.0 - 50.0) / t[-1] * t * t))).astype(np.float32)
    ck.check("sweep 50 Hz -> 10 kHz", fft.bank([x])[0], x)


@pytest.mark.parametrize("n", EDGE_LENGTHS)
def test_edge_lengths(fft, n):
    x = noise(n, 0.1, 100 + n)
    got = fft.bank([x])[0]
    assert got.shape == (80, _hip.lib().mcvc_audio_frames(n))
    ck.check("L=%d" % n, got, x)


def test_ragged_bank_equals_single_launches(fft):
    """One launch over 13 utterances of ragged lengths: every utterance bit-identical to its own single-utterance launch (a read across
    a neighbour at a reflected edge, or a frame landing at a wrong offset, would show), in both orders, and inside the gates."""
    xs = [noise(n, 0.1, 200 + i) + np.float32(0.05 * (i + 1)) for i, n in enumerate(BANK_LENGTHS)]     # a different offset each: neighbours differ at the joints
    single = [fft.bank([x])[0] for x in xs]
    for order in (list(range(len(xs))), list(range(len(xs)))[::-1]):
        got = fft.bank([xs[i] for i in order])
        assert len(got) == len(xs)
        for g, i in zip(got, order):
            assert g.shape == (80, _hip.lib().mcvc_audio_frames(BANK_LENGTHS[i])), i
            assert np.array_equal(g, single[i]), (i, BANK_LENGTHS[i], float(np.abs(g - single[i]).max()))
    for i in (3, 5, 7):
        ck.check("bank utterance %d L=%d" % (i, BANK_LENGTHS[i]), single[i], xs[i])


def test_vocoder_style_call_equals_the_bank(fft):
    x = np.stack([noise(5000, 0.1, 300 + b) for b in range(3)])
    want = np.stack(fft.bank(list(x)))
    xt = torch.from_numpy(x).cuda()
    for inp in (xt[:, None, :], xt):
        got = fft(inp)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, 80, 19) and got.is_contiguous()
        assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fft(torch.from_numpy(x))
    with pytest.raises(ValueError, match="at least 385 samples"):
        fft(xt[:, :384])


def _pcm(golden_dir, name):
    rate, pcm = wavfile.read(os.path.join(golden_dir, "audio", name))
    assert rate == 22050 and pcm.dtype == np.int16
    return pcm


def _speaker_folder(root, golden_dir, with_short=True):
    """<root>/SPK/{a,b,c_stereo,d_short}.wav -> the waveforms the checker sees (computed from the PCM here, not by read_wav)."""
    a, b = _pcm(golden_dir, "real_VCC2SF3.wav"), _pcm(golden_dir, "real_VCC2TF1.wav")
    stereo = np.stack([a, a // 2], axis=1)
    os.makedirs(os.path.join(root, "SPK", "sub"))
    wavfile.write(os.path.join(root, "SPK", "a.wav"), 22050, a)
    wavfile.write(os.path.join(root, "SPK", "sub", "b.wav"), 22050, b)             # sorted by path: after c_stereo.wav
    wavfile.write(os.path.join(root, "SPK", "c_stereo.wav"), 22050, stereo)
    waves = [a / 32768.0, stereo.astype(np.float64).mean(axis=1) / 32768.0, b / 32768.0]
    if with_short:
        wavfile.write(os.path.join(root, "SPK", "d_short.wav"), 22050, a[:10000])      # 39 frames < 64: dropped
    return [w.astype(np.float32) for w in waves]


def test_preprocess_cli_from_wavs(tmp_path, golden_dir):
    waves = _speaker_folder(str(tmp_path / "wavs"), golden_dir)
    preprocess_vcc2018.main(["--data_directory", str(tmp_path / "wavs"), "--preprocessed_data_directory", str(tmp_path / "out"), "--speaker_ids", "SPK"])
    mels, mean, std = load_speaker(str(tmp_path / "out"), "SPK")
    assert len(mels) == 3 and [m.shape for m in mels] == [(80, 224), (80, 224), (80, 225)]      # the short utterance is gone
    assert mean.shape == (80, 1) and std.shape == (80, 1)
    truths, G = [], 0.0
    for w in waves:
        truth, g_abs, _g_rel, _ = ck.gates(w)
        truths.append(truth.numpy())
        G = max(G, g_abs)
    want, wmean, wstd = preprocess_vcc2018.normalize_mels(truths)                      # float64 in, float64 statistics
    # Budget: every mel value is within G of the truth, so the mean moves by <= G and the std (1-Lipschitz in the sup norm) by <= G;
    # f32 = float32 summation of ~700 values of magnitude <= 5 in np.mean / np.std (pairwise: ~log2(N) roundings, taken as 16).
    f32 = 16 * 2.0 ** -24 * max(float(np.abs(t).max()) for t in truths)
    e_mean, e_std = float(np.abs(mean - wmean).max()), float(np.abs(std - wstd).max())
    print("preprocess CLI: G %.3e  mean err %.3e  std err %.3e (budget %.3e)" % (G, e_mean, e_std, G + f32))
    assert e_mean <= G + f32 and e_std <= G + f32
    for i, (m, w) in enumerate(zip(mels, want)):
        # z = (x - mean) / std: dz <= (dx + dmean + |z| dstd) / std, + the float32 rounding of z itself
        bound = 1.01 * (G + f32) * (2.0 + np.abs(w)) / wstd + 2.0 ** -23 * np.abs(w)
        err = np.abs(m.astype(np.float64) - w.astype(np.float64))
        print("preprocess CLI utterance %d: worst err / bound %.3f (max err %.3e)" % (i, float((err / bound).max()), float(err.max())))
        assert m.dtype == np.float32 and (err <= bound).all(), i


GATES = {"f32": (1e-3, 1e-3), "bf16": (2e-2, 6e-2)}        # test_hip_lengths.py: (whole tensor, worst frame) rel-L2


def _frame_errors(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    num, den = (got - ref).norm(dim=1), ref.norm(dim=1)
    return num / torch.maximum(den, 0.1 * den.pow(2).mean(dim=1, keepdim=True).sqrt())


def test_inference_cli_from_wav_dir(tmp_path, golden_dir):
    """python -m mask_cyclegan_vc.test --wav_dir: the written mels, normalised back, against Generator.infer on the checker's float64
    mels standardised with the source speaker's statistics, under the bars of test_hip_lengths.py."""
    from mask_cyclegan_vc import test as test_cli
    from mask_cyclegan_vc.model import Generator
    waves = _speaker_folder(str(tmp_path / "clips"), golden_dir, with_short=False)
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
    gp = orc.filler_params("G", 11)
    torch.save({"ckpt_info": {"epoch": 1}, "model_class": "Generator", "model_state": gp, "optimizer": None, "lr_scheduler": None},
               str(ck_dir / "00001_generator_A2B.pth.tar"))
    gen = Generator()
    gen.load_state_dict(gp, strict=True)
    gen.cuda()
    src = [((ck.log_mel(w).numpy() - stat["SPKA"]["mean"].astype(np.float64)) / stat["SPKA"]["std"].astype(np.float64)).astype(np.float32) for w in waves]
    mean, std = stat["SPKB"]["mean"].astype(np.float64), stat["SPKB"]["std"].astype(np.float64)
    for dtype in ("f32", "bf16"):
        test_cli.main(["--name", "wav_" + dtype, "--save_dir", str(tmp_path / "res"), "--preprocessed_data_dir", data, "--speaker_A_id", "SPKA",
                       "--speaker_B_id", "SPKB", "--ckpt_dir", str(ck_dir), "--load_epoch", "1", "--model_name", "generator_A2B", "--dtype", dtype,
                       "--wav_dir", str(tmp_path / "clips")])
        out = str(tmp_path / "res" / ("wav_" + dtype) / "converted_mel")
        assert len(os.listdir(out)) == 3
        for i, m in enumerate(src):
            with torch.no_grad():
                ref = gen.infer(torch.from_numpy(m)[None].cuda(), None, dtype).float().cpu()
            got = (np.load(os.path.join(out, "%d-converted_SPKA_to_SPKB.npy" % i)).astype(np.float64) - mean) / std
            assert got.shape == tuple(ref.shape[1:])
            whole = float((torch.from_numpy(got)[None] - ref.double()).norm() / ref.double().norm())
            worst = float(_frame_errors(got[None], ref).max())
            print("--wav_dir %-4s utterance %d T=%d: whole %.3e  worst frame %.3e" % (dtype, i, m.shape[1], whole, worst))
            assert whole <= GATES[dtype][0] and worst <= GATES[dtype][1], (dtype, i, whole, worst)


def test_bad_arguments_are_refused_and_write_nothing(fft):
    L = _hip.lib()
    x = torch.from_numpy(noise(5000, 0.1, 7)).cuda()
    offs = np.array([0, 5000], dtype=np.int32)
    fo = np.zeros(2, dtype=np.int32)
    nt = ctypes.c_int(0)
    tiles = np.zeros((1, 4), dtype=np.int32)
    assert L.mcvc_audio_plan(offs.ctypes.data, 1, fo.ctypes.data, tiles.ctypes.data, 1, ctypes.byref(nt)) == 0 and nt.value == 1 and fo[1] == 19
    spare = torch.zeros(8, dtype=torch.int32, device="cuda")
    spare[1:5] = torch.from_numpy(tiles[0]).cuda()                      # the same entry, 4 bytes off the 16-byte boundary
    td = torch.from_numpy(tiles).cuda()
    basis = fft.basis()
    out = torch.full((80, 19), 7.0, device="cuda")
    p, s = _hip.ptr, _hip.stream()
    good = (p(x), 5000, p(td), 1, p(basis), p(out), 19, s)
    for k, bad in ((0, None), (2, None), (4, None), (5, None),           # null wave / tiles / basis / out
                   (0, ctypes.c_void_p(x.data_ptr() + 2)),               # misaligned wave
                   (5, ctypes.c_void_p(out.data_ptr() + 1)),             # misaligned out
                   (2, ctypes.c_void_p(spare.data_ptr() + 4)),           # tiles off the 16-byte boundary
                   (4, ctypes.c_void_p(basis.data_ptr() + 4)),           # basis off the 16-byte boundary
                   (1, 384), (3, 0), (6, 0)):                            # too few samples, no work items, no frames
        args = list(good)
        args[k] = bad
        assert L.mcvc_audio_log_mel(*args) == MCVC_ERR_INVALID, k
    # a work list that does not describe this bank is skipped item by item, never followed out of the buffers
    wild = torch.tensor([[0, 6000, 0, 0], [4000, 5000, 0, 0], [0, 5000, 19, 0], [0, 5000, -1, 0], [0, 384, 0, 0], [-4, 5000, 0, 0]], dtype=torch.int32).cuda()
    assert L.mcvc_audio_log_mel(p(x), 5000, p(wild), 6, p(basis), p(out), 19, s) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(ValueError, match="at least 385 samples"):
        fft.bank([noise(5000, 0.1, 1), noise(384, 0.1, 2)])
    assert L.mcvc_audio_log_mel(*good) == 0                              # and the untouched arguments do work
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), fft.bank([x.cpu().numpy()])[0])
