"""GPU: the MelGAN decoder (csrc/vocoder_kernels.hip through mask_cyclegan_vc.vocoder.MelVocoder) and the inference driver's
--vocoder_ckpt path.

The checker is vocoder_checker.py: the network restated in torch with weight_norm on the CPU -- float64 is the truth, float32 the
reference's own arithmetic.  No trained MelGAN weights exist on the test machines: the weights are synthetic (torch default
initialisation at seed 0, weight_g x 1.7, biases in +-0.1), chosen so that the output is neither the last bias (gain 1) nor saturated
(gain 2); test_synthetic_weights_exercise_the_network asserts that on the float64 result alone.

Op level: every kernel path through ``mcvc_voc_layer`` against float64 F.conv1d / F.conv_transpose1d with the operand scaling and the
2e-5 rel-L2 gate of test_hip_ops.py; destinations are NaN-filled inside a guard band.

Whole decoder: the kernel may be at most 3x as far from the float64 result as the float32 CPU restatement is at the same input, as
whole-tensor rel-L2 and as max abs (the float32 restatement itself: 7.5e-7 .. 9.8e-7 rel-L2, 4e-7 .. 4e-6 max abs).  Every case prints
both pairs of figures before it asserts; DESIGN.md section 4 ("MelGAN decoder") records them."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy.io import wavfile

pytestmark = pytest.mark.gpu

import vocoder_checker as ck  # noqa: E402
import mcvc_oracle as orc  # noqa: E402  (filler parameters only)
from mask_cyclegan_vc import _hip  # noqa: E402
from mask_cyclegan_vc import vocoder as V  # noqa: E402
from mask_cyclegan_vc.utils import decode_melspectrogram  # noqa: E402

MCVC_ERR_INVALID, MCVC_ERR_WORKSPACE = 1001, 1002
GUARD = 64                                                  # floats either side of an op-level destination


@pytest.fixture(scope="module")
def voc():
    return V.MelVocoder().load_state_dict(ck.state_dict())


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def lrelu(x):
    return F.leaky_relu(x, 0.2)


def guarded(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def check_guarded(buf, y, ref, name):
    """every element written, none beyond the destination, rel-L2 under the op gate"""
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), name + ": guard band written"
    assert bool(torch.isfinite(y).all()), name + ": destination not fully written"
    assert tuple(y.shape) == tuple(ref.shape), name
    e = rel_l2(y, ref)
    print("%-28s rel-L2 %.3e" % (name, e))
    assert e < 2e-5, (name, e)


def operands(Cout, Cin, k, B, L, seed, transposed=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, L, generator=g)
    w = torch.randn(*((Cin, Cout, k) if transposed else (Cout, Cin, k)), generator=g) / np.sqrt(Cin * k)
    b = torch.randn(Cout, generator=g)
    return x, w, b


def test_synthetic_weights_exercise_the_network():
    a, _ = ck.decode(ck.synthetic_mel(1, 37, 5))
    b, _ = ck.decode(ck.synthetic_mel(1, 37, 6))
    rms, sat, sens = float(a.pow(2).mean().sqrt()), float((a.abs() > 0.99).double().mean()), float((a - b).norm() / a.norm())
    print("float64 synthetic decode at T = 37: rms %.3f, beyond 0.99 %.4f, input sensitivity %.3f" % (rms, sat, sens))
    assert 0.1 <= rms <= 0.6 and sat < 0.01 and sens > 0.2


CONV_CASES = [("first.L4", 80, 512, 7, 1, 4, False), ("first.L5", 80, 512, 7, 1, 5, False), ("first.L33", 80, 512, 7, 1, 33, False),
              ("d9.C256.L10", 256, 256, 3, 9, 10, True), ("d9.C32.L65", 32, 32, 3, 9, 65, True),
              ("d1.C64.L100", 64, 64, 3, 1, 100, True), ("d3.C64.L100", 64, 64, 3, 3, 100, True),
              ("d3.C32.L1100", 32, 32, 3, 3, 1100, True), ("d1.C128.L300", 128, 128, 3, 1, 300, False)]     # more than one time tile per configuration


@pytest.mark.parametrize("c", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_op_conv(c):
    name, Cin, Cout, k, d, L, act = c
    x, w, b = operands(Cout, Cin, k, 2, L, 1)
    xin = lrelu(x.double()) if act else x.double()
    ref = F.conv1d(F.pad(xin, ((k - 1) * d // 2,) * 2, "reflect"), w.double(), b.double(), dilation=d)
    buf, y = guarded(ref.shape)
    y = V.run_layer(V.KIND_CONV, x.cuda(), w, b, dilation=d, act_in=act, out=y)
    check_guarded(buf, y, ref, "conv " + name)


CONVT_CASES = [("r8.L4", 512, 256, 8, 4), ("r8.L37", 512, 256, 8, 37), ("r2.L4", 64, 32, 2, 4), ("r2.L37", 64, 32, 2, 37),
               ("r2.C128.L300", 128, 64, 2, 300), ("r2.L600", 64, 32, 2, 600)]


@pytest.mark.parametrize("c", CONVT_CASES, ids=[c[0] for c in CONVT_CASES])
def test_op_transposed_conv(c):
    name, Cin, Cout, r, L = c
    x, w, b = operands(Cout, Cin, 2 * r, 2, L, 2, transposed=True)
    ref = F.conv_transpose1d(lrelu(x.double()), w.double(), b.double(), stride=r, padding=r // 2 + r % 2, output_padding=r % 2)
    assert ref.shape[-1] == r * L
    buf, y = guarded(ref.shape)
    y = V.run_layer(V.KIND_CONVT, x.cuda(), w, b, r=r, act_in=True, out=y)
    check_guarded(buf, y, ref, "transposed " + name)


@pytest.mark.parametrize("dim,L", [(128, 45), (32, 77), (32, 1061), (64, 259)])
def test_op_stacked_residual_product(dim, L):
    x, w0, b0 = operands(dim, dim, 1, 2, L, 3)
    h, w1, b1 = operands(dim, dim, 1, 2, L, 4)
    ref = F.conv1d(x.double(), w0.double(), b0.double()) + F.conv1d(lrelu(h.double()), w1.double(), b1.double())
    buf, y = guarded(ref.shape)
    y = V.run_layer(V.KIND_STACK, x.cuda(), w0, b0, x1=h.cuda(), w1=w1, b1=b1, out=y)
    check_guarded(buf, y, ref, "stacked dim %d L %d" % (dim, L))


@pytest.mark.parametrize("L", [7, 1025])
def test_op_last_conv_tanh(L):
    x, w, b = operands(1, 32, 7, 2, L, 5)
    x, b = 2.0 * x, 0.1 * b                                  # pre-activations of order 1: tanh neither linear nor saturated
    ref = torch.tanh(F.conv1d(F.pad(lrelu(x.double()), (3, 3), "reflect"), w.double(), b.double()))[:, 0]
    buf, y = guarded(ref.shape)
    y = V.run_layer(V.KIND_LAST, x.cuda(), w, b, out=y)
    check_guarded(buf, y, ref, "last conv + tanh L %d" % L)


def test_op_refusals():
    x, w, b = operands(32, 32, 3, 1, 9, 6)
    with pytest.raises(RuntimeError):                        # reflection of 9 needs 10 samples
        V.run_layer(V.KIND_CONV, x.cuda(), w, b, dilation=9)
    with pytest.raises(RuntimeError):
        V.run_layer(V.KIND_CONV, x, w, b)                    # a CPU tensor


_b1 = {}


def single(voc, T, seed):
    if (T, seed) not in _b1:
        _b1[(T, seed)] = voc.inverse(ck.synthetic_mel(1, T, seed).cuda()).cpu()
    return _b1[(T, seed)]


@pytest.mark.parametrize("B,T", [(1, 4), (2, 5), (2, 37), (1, 64)])
def test_whole_decoder(voc, B, T):
    mel = torch.cat([ck.synthetic_mel(1, T, 10 + j) for j in range(B)])
    ref64, ref32 = ck.decode(mel)
    got = voc.inverse(mel.cuda())
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (B, 256 * T)
    again = voc.inverse(mel.cuda())
    assert torch.equal(got, again), "two runs differ"
    for j in range(B):
        assert torch.equal(got[j].cpu(), single(voc, T, 10 + j)[0]), "row %d differs from its B = 1 result" % j
    (k_l2, k_abs), (f_l2, f_abs) = ck.distances(got, ref64), ck.distances(ref32, ref64)
    print("decoder B=%d T=%d: kernel rel-L2 %.3e max-abs %.3e | float32 CPU rel-L2 %.3e max-abs %.3e | ratios %.2f %.2f"
          % (B, T, k_l2, k_abs, f_l2, f_abs, k_l2 / f_l2, k_abs / f_abs))
    assert k_l2 <= 3.0 * f_l2 and k_abs <= 3.0 * f_abs, (k_l2, f_l2, k_abs, f_abs)


def test_decode_melspectrogram_is_the_references_two_lines(voc):
    mel = ck.synthetic_mel(1, 9, 21)[0].cuda()
    mean, std = torch.full((80, 1), -2.0, device="cuda"), torch.full((80, 1), 1.5, device="cuda")
    got = decode_melspectrogram(voc, mel, mean, std)
    assert tuple(got.shape) == (1, 256 * 9) and torch.equal(got, voc.inverse((mel * std + mean)[None]))


def test_refusals(voc):
    with pytest.raises(ValueError):
        voc.inverse(ck.synthetic_mel(1, 3, 1).cuda())
    with pytest.raises(RuntimeError):
        voc.inverse(ck.synthetic_mel(1, 8, 1))
    with pytest.raises(RuntimeError):
        V.MelVocoder().inverse(ck.synthetic_mel(1, 8, 1).cuda())       # no weights loaded
    L = _hip.lib()
    B, T = 1, 8
    mel = ck.synthetic_mel(B, T, 1).cuda()
    n = L.mcvc_voc_workspace_floats(B, T)
    ws = torch.full((n,), float("nan"), device="cuda")
    out = torch.full((B, 256 * T), float("nan"), device="cuda")
    args = lambda floats, b, t: (_hip.ptr(voc.packed), _hip.ptr(mel), _hip.ptr(out), _hip.ptr(ws), floats, b, t, _hip.stream())
    assert L.mcvc_voc_decode(*args(n - 1, B, T)) == MCVC_ERR_WORKSPACE
    assert L.mcvc_voc_decode(*args(n, B, 3)) == MCVC_ERR_INVALID
    assert L.mcvc_voc_decode(*args(n, 0, T)) == MCVC_ERR_INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws).all()) and bool(torch.isnan(out).all()), "a refused call launched something"
    assert L.mcvc_voc_decode(*args(n, B, T)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, voc.inverse(mel))


def test_inference_cli_writes_wavs(tmp_path, golden_dir, voc):
    """python -m mask_cyclegan_vc.test --wav_dir ... --vocoder_ckpt: the reference's wav pair per utterance, bit-equal to
    MelVocoder.inverse of the written mels; without the flag no converted_audio and the same .npy files."""
    from data_preprocessing.audio2mel import read_wav
    from mask_cyclegan_vc import test as test_cli
    clips = tmp_path / "clips"
    clips.mkdir()
    for i, n in enumerate(("real_VCC2SF3.wav", "real_VCC2TF1.wav")):       # two short cuts of the golden recordings: 24 and 31 frames
        x = read_wav(os.path.join(golden_dir, "audio", n))
        wavfile.write(str(clips / ("%d.wav" % i)), 22050, x[4000:4000 + 256 * (24 + 7 * i) + 100])
    data = str(tmp_path / "data")
    rs = np.random.RandomState(4)
    for spk in ("SPKA", "SPKB"):
        os.makedirs(os.path.join(data, spk))
        with open(os.path.join(data, spk, "%s_normalized.pickle" % spk), "wb") as fh:
            pickle.dump([rs.randn(80, 64).astype(np.float32)], fh)
        np.savez(os.path.join(data, spk, "%s_norm_stat.npz" % spk), mean=(-2.0 + 0.3 * rs.randn(80, 1)).astype(np.float32),
                 std=(1 + 0.2 * rs.rand(80, 1)).astype(np.float32))
    ck_dir = tmp_path / "ckpts"
    ck_dir.mkdir()
    torch.save({"ckpt_info": {"epoch": 1}, "model_class": "Generator", "model_state": orc.filler_params("G", 11), "optimizer": None, "lr_scheduler": None},
               str(ck_dir / "00001_generator_A2B.pth.tar"))
    torch.save(ck.state_dict(), str(tmp_path / "melgan.pt"))
    common = ["--save_dir", str(tmp_path / "res"), "--preprocessed_data_dir", data, "--speaker_A_id", "SPKA", "--speaker_B_id", "SPKB",
              "--ckpt_dir", str(ck_dir), "--load_epoch", "1", "--model_name", "generator_A2B", "--wav_dir", str(clips)]
    test_cli.main(["--name", "with"] + common + ["--vocoder_ckpt", str(tmp_path / "melgan.pt")])
    test_cli.main(["--name", "without"] + common)
    assert not os.path.exists(str(tmp_path / "res" / "without" / "converted_audio"))
    mel_dir, wav_dir = tmp_path / "res" / "with" / "converted_mel", tmp_path / "res" / "with" / "converted_audio"
    assert sorted(os.listdir(str(wav_dir))) == sorted("%d-%s_SPKA_to_SPKB.wav" % (i, k) for i in range(2) for k in ("converted", "original"))
    for i in range(2):
        name = "%d-converted_SPKA_to_SPKB.npy" % i
        mel = np.load(str(mel_dir / name))
        assert np.array_equal(mel, np.load(str(tmp_path / "res" / "without" / "converted_mel" / name)))
        T_src = 24 + 7 * i
        T = mel.shape[1]                                     # (the generator rounds 31 frames up to 32)
        assert T == (T_src + 3) // 4 * 4
        want = voc.inverse(torch.from_numpy(mel)[None].cuda())[0].cpu().numpy()
        for kind, frames in (("converted", T), ("original", T_src)):
            rate, wav = wavfile.read(str(wav_dir / ("%d-%s_SPKA_to_SPKB.wav" % (i, kind))))
            assert rate == 22050 and wav.dtype == np.float32 and wav.shape == (256 * frames,), (i, kind)
            assert np.isfinite(wav).all() and np.abs(wav).max() <= 1.0
        _, wav = wavfile.read(str(wav_dir / ("%d-converted_SPKA_to_SPKB.wav" % i)))
        assert np.array_equal(wav, want), "utterance %d: the wav is not the decode of the written mel" % i
