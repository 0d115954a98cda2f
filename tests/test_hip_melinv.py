"""GPU: the mel inversion (csrc/melinv_kernels.hip via mask_cyclegan_vc.melinv.MelInverter), ``GriffinLimVocoder(mel_inverse="nnls")``
and the ``--gl_mel_inverse`` / ``--gl_mel_iter`` flags of the inference driver.

The checker is melinv_checker.py: the definition in numpy with dense products -- float64 is the truth, float32 the yardstick.  The
gate is per frame: |hip - f64| <= max(2e-6 x that frame's largest float64 magnitude, 4 x the float32 checker's largest distance from
float64 in that frame).  2e-6 is the project's floor for unit-scale signals (scaled: magnitudes reach about 100), 4 its factor for long
chains.  The problem is underdetermined, so a float32 state drifts along the null space of the basis (float32 against float64 grows
from 1e-6 to 3e-5 of the frame maximum between 16 and 128 iterations): the gate follows the float32 restatement, not a constant.  The
kernel carries its state in float64 and stays near the floor (profiles/melinv_error.json, recorded by this file with
MCVC_MELINV_ERROR_JSON=<path>).  Every test prints its figures before it asserts."""
import ctypes
import json
import os
import pickle

import numpy as np
import pytest
import torch
from scipy.io import wavfile

pytestmark = pytest.mark.gpu

import audio_checker as ack  # noqa: E402
import melinv_checker as ck  # noqa: E402
import mcvc_oracle as orc  # noqa: E402  (filler parameters only)
from data_preprocessing.audio2mel import Audio2Mel, read_wav  # noqa: E402
from mask_cyclegan_vc import _hip  # noqa: E402
from mask_cyclegan_vc.griffinlim import ZERO_PHASE, GriffinLimVocoder  # noqa: E402
from mask_cyclegan_vc.melinv import MelInverter  # noqa: E402

MCVC_ERR_INVALID = 1001
TF = 16                                                     # frames of a workgroup's tile (csrc/melinv_kernels.hip)
SHAPES = [(1, 1), (1, TF - 1), (1, TF), (1, TF + 1), (2, 2 * TF + 5), (3, 2 * TF + 3)]
ITERS = [1, 2, 8, 64]
WORST = {}


@pytest.fixture(scope="module")
def inv():
    return MelInverter()


@pytest.fixture(scope="module")
def clips(golden_dir):
    """The float64 log-mels [80, T] of the two committed recordings, by the front-end's checker."""
    return [ack.log_mel(read_wav(os.path.join(golden_dir, "audio", n))).numpy() for n in ("real_VCC2SF3.wav", "real_VCC2TF1.wav")]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def mixed_input(clips, B, T, seed):
    """[B, 80, T] float32: frame f = b T + t is, by f % 4, a frame of a recording (each sample has its own clip and offset), a random
    log-mel in [-5, 2], the front-end's floor (-5 everywhere), or the floor with one hot band."""
    rs = np.random.RandomState(seed)
    x = np.empty((B, 80, T), dtype=np.float32)
    for b in range(B):
        clip = clips[b % 2]
        x[b] = clip[:, 30 + 40 * b:30 + 40 * b + T]
        for t in range(T):
            kind = (b * T + t) % 4
            if kind == 1:
                x[b, :, t] = rs.uniform(-5.0, 2.0, 80)
            elif kind == 2:
                x[b, :, t] = -5.0
            elif kind == 3:
                x[b, :, t] = -5.0
                x[b, (7 * (b * T + t)) % 80, t] = rs.uniform(0.0, 2.0)
    return x


@pytest.fixture(scope="module")
def cases(clips):
    """(B, T) -> (input, {n_iter: (float64 result, float32 checker's result)}), computed once."""
    out = {}
    for B, T in SHAPES:
        x = mixed_input(clips, B, T, 100 * B + T)
        out[(B, T)] = (x, {n: (ck.solve(x, n), ck.solve(x, n, np.float32)) for n in [0] + ITERS})
    kinds = np.stack([mixed_input(clips, 1, 4, 9)[0, :, k:k + 1] for k in range(4)])      # [4, 80, 1]: one frame of each kind, T = 1
    out["kinds"] = (kinds, {n: (ck.solve(kinds, n), ck.solve(kinds, n, np.float32)) for n in [0] + ITERS})
    return out


def run(inv, x, n_iter):
    got = inv(dev(x), n_iter=n_iter)
    B, T = x.shape[0], x.shape[2]
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (B, 513, T) and got.is_contiguous() and not got.requires_grad
    return got.cpu().numpy()


def gate(tag, got, truth, ref32):
    assert np.isfinite(got).all() and (got >= 0).all(), tag
    d, g = ck.frame_gate(got, truth, ref32)
    d32 = np.abs(ref32.astype(np.float64) - truth).max(axis=1)
    peak = np.abs(truth).max(axis=1)
    fig = dict(d_over_gate=float((d / g).max()), d_over_peak=float((d / peak).max()), f32_over_peak=float((d32 / peak).max()),
               d_over_f32=float((d / np.maximum(d32, 1e-300)).max()))
    print("%-34s frames %3d  worst |hip - f64| / gate %.3f  / frame peak %.2e  (float32 checker / peak %.2e, hip / float32 checker <= %.2f)"
          % (tag, d.size, fig["d_over_gate"], fig["d_over_peak"], fig["f32_over_peak"], fig["d_over_f32"]))
    WORST[tag] = fig
    assert (d <= g).all(), (tag, float((d / g).max()))


# ---- 1. the start value ------------------------------------------------------------------------------------------------------------------------
def test_1_start_value_is_the_decoders(inv, clips):
    """n_iter = 0 is max(0, P y) as gl_init_kernel computes it: read from the decoder's own workspace (its last section, rows of 514 per
    frame: the comment at the top of csrc/griffinlim_kernels.hip), and through the two decodes, which must agree bit for bit."""
    L = _hip.lib()
    gl = GriffinLimVocoder()
    B, T = 2, TF + 3
    x = dev(mixed_input(clips, B, T, 1))
    M0 = inv(x, n_iter=0)
    n = L.mcvc_gl_workspace_floats(B, T)
    ws = torch.zeros(n, dtype=torch.float32, device="cuda")
    wav = torch.empty(B, 256 * T, dtype=torch.float32, device="cuda")
    assert L.mcvc_gl_decode(_hip.ptr(x), 0, None, _hip.ptr(gl.tables()), _hip.ptr(wav), _hip.ptr(ws), n, B, T, 0, 0.99, _hip.stream()) == 0
    torch.cuda.synchronize()
    mag = ws[3 * B * T * 1024:].view(B, T, 514)[:, :, :513].permute(0, 2, 1).contiguous()
    assert float(mag.max()) > 0 and torch.equal(M0, mag)
    a = gl.inverse(x, angles=ZERO_PHASE, n_iter=0)
    b = gl.from_magnitude(M0, angles=ZERO_PHASE, n_iter=0)
    assert torch.equal(a, b) and torch.equal(a, wav)
    nn = GriffinLimVocoder(mel_inverse="nnls", mel_iter=0)                   # and the class with zero solver steps is the default class
    assert torch.equal(nn.inverse(x, n_iter=2), gl.inverse(x, n_iter=2))
    truth, ref32 = ck.solve(x.cpu().numpy(), 0), ck.solve(x.cpu().numpy(), 0, np.float32)
    gate("1 start value B=%d T=%d" % (B, T), M0.cpu().numpy(), truth, ref32)


# ---- 2. element by element against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_iter", ITERS)
@pytest.mark.parametrize("B,T", SHAPES)
def test_2_against_float64(inv, cases, B, T, n_iter):
    x, want = cases[(B, T)]
    gate("2 B=%d T=%d n_iter=%d" % (B, T, n_iter), run(inv, x, n_iter), *want[n_iter])
    path = os.environ.get("MCVC_MELINV_ERROR_JSON")
    if path:                                                                  # (how profiles/melinv_error.json was recorded)
        with open(path, "w") as fh:
            json.dump(dict(cases=WORST, note="per case, the largest over its frames; cases of test_hip_melinv.py run so far"), fh, indent=1)


@pytest.mark.parametrize("n_iter", [0] + ITERS)
def test_2_one_frame_of_each_kind(inv, cases, n_iter):
    """B = 4, T = 1: a frame of speech, a random one, the floor, one hot band -- each alone in its tile."""
    x, want = cases["kinds"]
    got = run(inv, x, n_iter)
    gate("2 kinds n_iter=%d" % n_iter, got, *want[n_iter])
    assert got[:, 0, 0].tolist() == run(inv, x, 0)[:, 0, 0].tolist() and got[:, 512, 0].tolist() == run(inv, x, 0)[:, 512, 0].tolist()  # bins in no filter


# ---- 3. batching ------------------------------------------------------------------------------------------------------------------------------
def test_3_batches_permutations_and_lengths(inv, clips):
    B, T, n = 3, 2 * TF + 3, 8
    x = dev(mixed_input(clips, B, T, 3))
    whole = inv(x, n_iter=n)
    assert torch.equal(inv(x, n_iter=n), whole)
    for b in range(B):
        assert torch.equal(inv(x[b:b + 1], n_iter=n)[0], whole[b]), b
    perm = torch.from_numpy(np.random.RandomState(4).permutation(T)).cuda()
    assert torch.equal(inv(x[:, :, perm].contiguous(), n_iter=n), whole[:, :, perm])            # a frame does not care where it stands
    for T2 in (1, TF - 1, TF, TF + 1, T - 1):
        assert torch.equal(inv(x[:, :, :T2].contiguous(), n_iter=n), whole[:, :, :T2]), T2      # nor how long its utterance is
        assert torch.equal(inv(x[:, :, T - T2:].contiguous(), n_iter=n), whole[:, :, T - T2:]), T2
    assert torch.equal(MelInverter(n_iter=n)(x), whole) and torch.equal(MelInverter(n_iter=n).inv(x), whole)
    assert not torch.equal(inv(x, n_iter=n + 1), whole)
    assert torch.equal(inv(x.double(), n_iter=n), whole)                                        # any real dtype in, float32 out
    with pytest.raises(RuntimeError, match="no CPU path"):
        inv(x.cpu())
    for bad in (-1, 513):
        with pytest.raises(ValueError):
            inv(x, n_iter=bad)
    with pytest.raises(ValueError):
        inv(x[:, :79])


# ---- 4. output ----------------------------------------------------------------------------------------------------------------------------------
def test_4_output_is_overwritten_and_refusals_write_nothing(inv, clips):
    L = _hip.lib()
    B, T = 2, TF + 1
    x = dev(mixed_input(clips, B, T, 5))
    tables = inv.tables()
    out = torch.full((B * 513 * T + 8,), float("nan"), device="cuda")
    p, s = _hip.ptr, _hip.stream()
    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    good = [p(x), p(tables), p(out), B, T, 8, s]
    for k, bad in ((0, None), (1, None), (2, None), (0, off(x, 2)), (1, off(tables, 4)), (2, off(out, 1)), (3, 0), (4, 0), (5, -1), (5, 513),
                   (3, 65536), (4, (1 << 20) + 1)):
        args = list(good)
        args[k] = bad
        assert L.mcvc_melinv_solve(*args) == MCVC_ERR_INVALID, (k, bad)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                                      # refused: untouched
    assert L.mcvc_melinv_solve(*good) == 0
    torch.cuda.synchronize()
    body = out[:B * 513 * T].view(B, 513, T)
    assert bool(torch.isfinite(body).all()) and bool((body >= 0).all()) and bool(torch.isnan(out[B * 513 * T:]).all())
    assert torch.equal(body, inv(x, n_iter=8))


# ---- 5. the golden clips at the default --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [0, 1])
def test_5_golden_clips_at_64_iterations(inv, clips, clip):
    """|| B M - y || / || y ||, in float64 from the kernel's output, <= 1 / 10 of the float64 checker's value for the clamp."""
    x = clips[clip][None].astype(np.float32)
    assert inv.n_iter == 64
    got = inv(dev(x)).cpu().numpy()
    res, res0, res64 = ck.mel_residual(got, x), ck.mel_residual(ck.solve(x, 0), x), ck.mel_residual(ck.solve(x, 64), x)
    print("5 clip %d T=%d: mel residual kernel %.3e, float64 checker at 64 iterations %.3e, the clamp %.3e (kernel / clamp = 1 / %.0f)"
          % (clip, x.shape[2], res, res64, res0, res0 / res))
    assert (got >= 0).all() and res <= res0 / 10.0


# ---- 6. the driver ------------------------------------------------------------------------------------------------------------------------------
def test_6_inference_cli(tmp_path, golden_dir):
    """--griffin_lim 2 on the two committed recordings with a tiny checkpoint: --gl_mel_inverse pinv writes the bytes a run without the
    flag writes; nnls with 8 solver steps writes the WAVs the class gives when called directly, and they differ from the pinv ones."""
    from mask_cyclegan_vc import test as test_cli
    wav_dir = os.path.join(golden_dir, "audio")
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
              "--ckpt_dir", str(ck_dir), "--load_epoch", "1", "--model_name", "generator_A2B", "--wav_dir", wav_dir, "--griffin_lim", "2"]
    test_cli.main(["--name", "plain"] + common)
    test_cli.main(["--name", "pinv", "--gl_mel_inverse", "pinv"] + common)
    test_cli.main(["--name", "nnls", "--gl_mel_inverse", "nnls", "--gl_mel_iter", "8"] + common)
    res = lambda name, *parts: str(tmp_path.joinpath("res", name, *parts))
    wavs = sorted("%d-%s_SPKA_to_SPKB.wav" % (i, k) for i in (0, 1) for k in ("converted", "original"))
    mels = sorted("%d-converted_SPKA_to_SPKB.npy" % i for i in (0, 1))
    for name in ("plain", "pinv", "nnls"):
        assert sorted(os.listdir(res(name))) == ["converted_audio", "converted_mel", "test_args.json"]
        assert sorted(os.listdir(res(name, "converted_audio"))) == wavs and sorted(os.listdir(res(name, "converted_mel"))) == mels
    read = lambda *parts: open(res(*parts), "rb").read()
    for f in wavs:
        assert read("pinv", "converted_audio", f) == read("plain", "converted_audio", f), f
        assert read("nnls", "converted_audio", f) != read("plain", "converted_audio", f), f
    for f in mels:
        assert read("pinv", "converted_mel", f) == read("plain", "converted_mel", f) == read("nnls", "converted_mel", f), f
    gl = GriffinLimVocoder(n_iter=2, mel_inverse="nnls", mel_iter=8)
    fft = Audio2Mel()
    for i, w in enumerate(read_wav(os.path.join(wav_dir, n)) for n in ("real_VCC2SF3.wav", "real_VCC2TF1.wav")):
        (mel,) = fft.bank([w])
        src = (((mel - stat["SPKA"]["mean"]) / stat["SPKA"]["std"]).astype(np.float32) * stat["SPKA"]["std"] + stat["SPKA"]["mean"]).astype(np.float32)
        conv = np.load(res("nnls", "converted_mel", "%d-converted_SPKA_to_SPKB.npy" % i))
        for kind, m in (("original", src), ("converted", conv)):
            rate, wav = wavfile.read(res("nnls", "converted_audio", "%d-%s_SPKA_to_SPKB.wav" % (i, kind)))
            assert rate == 22050 and wav.dtype == np.float32 and wav.shape == (256 * m.shape[1],) and np.isfinite(wav).all()
            assert np.array_equal(wav, gl.inverse(dev(m[None]))[0].cpu().numpy()), (i, kind)
            rate, plain = wavfile.read(res("plain", "converted_audio", "%d-%s_SPKA_to_SPKB.wav" % (i, kind)))
            print("6 CLI utterance %d %s: nnls(8) and pinv waveforms differ by %.3e of the peak" % (i, kind, np.abs(wav - plain).max() / np.abs(plain).max()))
            assert not np.array_equal(wav, plain)
