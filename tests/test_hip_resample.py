"""GPU: the polyphase resampler (csrc/resample_kernels.hip via data_preprocessing.resample.Resampler), ``Audio2Mel.bank_at_rates`` and the
``--gpu_resample`` / ``--out_sample_rate`` paths of the two command-line drivers.

The truth is tests/resample_checker.py: the float64 direct sum fed the same float32 input and the float64 taps (pinned to scipy at 1e-12 by
tests/test_host_resample.py).  The gate is per output element and derived, not measured:

    |got - ref| <= 1.01 (n_k + 2) 2^-24 sum_i |x_i| |h_j|

n_k terms: one rounding per tap (float64 -> float32), one per product, n_k for the sums -- it holds for any summation order, with or without
FMA.  Every case prints its largest error / gate before it asserts; MCVC_RESAMPLE_ERROR_JSON=<path> records the per-case maxima (how
profiles/resample_error.json was made)."""
import ctypes
import json
import os
import pickle

import numpy as np
import pytest
import torch
from scipy import signal
from scipy.io import wavfile

pytestmark = pytest.mark.gpu

import mcvc_oracle as orc  # noqa: E402  (filler parameters only)
import resample_checker as ck  # noqa: E402
from data_preprocessing import preprocess_vcc2018  # noqa: E402
from data_preprocessing.audio2mel import Audio2Mel, num_frames, read_wav  # noqa: E402
from data_preprocessing.resample import Resampler  # noqa: E402
from mask_cyclegan_vc import _hip  # noqa: E402
from mask_cyclegan_vc.train import load_speaker  # noqa: E402

MCVC_ERR_INVALID = 1001
RATIOS = [(441, 320), (147, 320), (1, 2), (320, 441), (320, 147), (2, 1), (147, 640)]
WORST = {}


@pytest.fixture(scope="module")
def rs():
    return Resampler()


def tile():
    return _hip.lib().mcvc_resample_tile_samples()


def length_for(n_out, up, down):
    """The shortest input with at least ``n_out`` outputs: exactly n_out when down >= up; when upsampling not every count exists and the
    next one above is taken."""
    n = max(1, (n_out - 1) * down // up)
    while ck.out_len(n, up, down) < n_out:
        n += 1
    return n


def lengths_of(up, down):
    half, T = 10 * max(up, down), tile()
    short = (half - 1) // up                                   # n_in up < half: the utterance is shorter than half the filter
    assert short >= 1 and short * up < half
    return [1, 2, short] + [length_for(n, up, down) for n in (T - 1, T, T + 1, 2 * T + 1)] + [20001]


def noise(n, seed, dc=0.0):
    return (0.1 * np.random.RandomState(seed).randn(n)).astype(np.float32) + np.float32(dc)


def run(rs, xs, up, down):
    """One launch over the utterances ``xs`` -> list of float32 numpy (rates down -> up Hz have the ratio up / down)."""
    return rs.bank(xs, down, up, to_host=True)


def record(case, worst):
    WORST[case] = max(WORST.get(case, 0.0), worst)
    path = os.environ.get("MCVC_RESAMPLE_ERROR_JSON")
    if path:
        with open(path, "w") as fh:
            json.dump(dict(worst_error_over_gate=WORST, gate="1.01 (n_k + 2) 2^-24 sum |x_i| |h_j| per output, against the float64 checker",
                           note="largest over the cases of tests/test_hip_resample.py run so far"), fh, indent=1)


# ---- 1. element by element against float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up,down", RATIOS)
def test_lengths_against_float64(rs, up, down):
    L = _hip.lib()
    T = tile()
    lens = lengths_of(up, down)
    if down >= up:
        assert [ck.out_len(n, up, down) for n in lens[3:7]] == [T - 1, T, T + 1, 2 * T + 1]
    worst = 0.0
    for n in lens:
        x = noise(n, 1000 + n, dc=0.05)
        (got,) = run(rs, [x], up, down)
        assert got.shape == (L.mcvc_resample_out_samples(n, up, down),)
        worst = max(worst, ck.check("noise + DC n_in=%d" % n, got, x, up, down))
    for n in (lens[2], lens[4], lens[6]):                      # shorter than the filter, one full row, three rows
        for where in (0, n - 1):
            x = np.zeros(n, dtype=np.float32)
            x[where] = 1.0
            (got,) = run(rs, [x], up, down)
            worst = max(worst, ck.check("impulse at %d of %d" % (where, n), got, x, up, down))
            assert np.abs(got).max() > 0
    record("%d/%d" % (up, down), worst)


# ---- 2. the ragged bank ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up,down", [(441, 320), (147, 320), (320, 441)])
def test_ragged_bank_equals_single_launches(rs, up, down):
    """A dozen utterances in one launch, a different DC offset each so that neighbours differ at the joints, in both orders: every utterance
    bit-identical to its own launch (a neighbour's sample inside the filter's reach would show) and inside the gate; the guard floats on
    both sides of the output buffer stay as they were."""
    L = _hip.lib()
    lens = lengths_of(up, down) + [3, 5000, 777, 1]
    xs = [noise(n, 2000 + i, dc=0.05 * (i + 1)) for i, n in enumerate(lens)]
    single = [run(rs, [x], up, down)[0] for x in xs]
    worst = max(ck.check("bank utterance %d n_in=%d" % (i, lens[i]), single[i], xs[i], up, down) for i in range(len(xs)))
    record("bank %d/%d" % (up, down), worst)
    for order in (list(range(len(xs))), list(range(len(xs)))[::-1]):
        got = run(rs, [xs[i] for i in order], up, down)
        assert len(got) == len(xs)
        for g, i in zip(got, order):
            assert np.array_equal(g, single[i]), (i, lens[i], float(np.abs(g - single[i]).max()) if g.shape == single[i].shape else g.shape)
    # the same launch through the C ABI into a buffer with guards
    GUARD = 64
    order = list(range(len(xs)))
    offs = np.concatenate([[0], np.cumsum([lens[i] for i in order])]).astype(np.int32)
    oo = np.zeros(len(order) + 1, dtype=np.int32)
    nt = ctypes.c_int(0)
    assert L.mcvc_resample_plan(offs.ctypes.data, len(order), up, down, oo.ctypes.data, None, 0, ctypes.byref(nt)) == 0
    tiles = torch.zeros(nt.value, 8, dtype=torch.int32).pin_memory()
    assert L.mcvc_resample_plan(offs.ctypes.data, len(order), up, down, oo.ctypes.data, tiles.data_ptr(), nt.value, ctypes.byref(nt)) == 0
    total = int(oo[-1])
    wave = torch.from_numpy(np.concatenate([xs[i] for i in order])).cuda()
    buf = torch.full((total + 2 * GUARD,), 7.0, device="cuda")
    y = buf[GUARD:GUARD + total]
    assert L.mcvc_resample_run(_hip.ptr(wave), int(offs[-1]), ctypes.c_void_p(tiles.data_ptr()), nt.value, _hip.ptr(rs.table(up, down)), up, down,
                               _hip.ptr(y), total, _hip.stream()) == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 7.0).all() and (host[GUARD + total:] == 7.0).all()
    for k, i in enumerate(order):
        assert np.array_equal(host[GUARD + oo[k]:GUARD + oo[k + 1]], single[i]), i


# ---- 3. the Resampler's calls ----------------------------------------------------------------------------------------------------------
def test_batched_call_equals_the_bank(rs):
    x = np.stack([noise(5000, 300 + b, dc=0.01 * b) for b in range(3)])
    xt = torch.from_numpy(x).cuda()
    for r_in, r_out in ((16000, 22050), (22050, 16000), (48000, 22050)):
        want = np.stack(rs.bank(list(x), r_in, r_out, to_host=True))
        got = rs(xt, r_in, r_out)
        assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want)
        dev, offs = rs.bank([xt[b] for b in range(3)], r_in, r_out)        # device waveforms in, device bank out
        assert dev.is_cuda and offs.tolist() == [0, want.shape[1], 2 * want.shape[1], 3 * want.shape[1]]
        assert np.array_equal(dev.cpu().numpy(), want.reshape(-1))
    assert rs(xt, 22050, 22050) is xt and rs(xt, 44100, 44100) is xt      # equal rates: the input, no launch
    same, offs = rs.bank(list(x), 22050, 22050)
    assert np.array_equal(same.cpu().numpy(), x.reshape(-1)) and offs.tolist() == [0, 5000, 10000, 15000]


def test_refusals_leave_the_output_alone(rs):
    L = _hip.lib()
    assert L.mcvc_resample_max_factor() == 640
    x = noise(5000, 7)
    xt = torch.from_numpy(x).cuda()
    with pytest.raises(RuntimeError, match="no CPU path"):
        rs(torch.from_numpy(x)[None], 16000, 22050)
    with pytest.raises(ValueError, match="limit of 640"):
        rs(xt[None], 22050, 641)                                          # 641 / 22050 in lowest terms
    with pytest.raises(ValueError, match="limit of 640"):
        rs.bank([x], 22050 * 641, 22050)
    with pytest.raises(ValueError, match=r"\[B, L\]"):
        rs(xt, 16000, 22050)
    up, down = 441, 320
    offs = np.array([0, 5000], dtype=np.int32)
    oo = np.zeros(2, dtype=np.int32)
    nt = ctypes.c_int(0)
    assert L.mcvc_resample_plan(offs.ctypes.data, 1, up, down, oo.ctypes.data, None, 0, ctypes.byref(nt)) == 0
    good_tiles = torch.zeros(nt.value, 8, dtype=torch.int32).pin_memory()
    assert L.mcvc_resample_plan(offs.ctypes.data, 1, up, down, oo.ctypes.data, good_tiles.data_ptr(), nt.value, ctypes.byref(nt)) == 0
    total = int(oo[1])
    out = torch.full((total,), 7.0, device="cuda")
    table = rs.table(up, down)

    def call(tiles, x_ptr=_hip.ptr(xt), table_ptr=_hip.ptr(table), y_ptr=_hip.ptr(out), n_tiles=None, u=up, d=down, n_in=5000, n_out=total):
        return L.mcvc_resample_run(x_ptr, n_in, None if tiles is None else ctypes.c_void_p(tiles.data_ptr()), nt.value if n_tiles is None else n_tiles,
                                   table_ptr, u, d, y_ptr, n_out, _hip.stream())
    TILE = tile()
    wild = []
    for col, value in ((0, -1), (0, 1), (1, 0), (1, 5001), (2, -1), (2, total), (3, 0), (3, TILE + 1), (4, -1), (5, -1), (5, up), (2, 2 ** 30), (0, 2 ** 30)):
        t = good_tiles.clone().pin_memory()
        t[-1, col] = value                                                # one wild field in the last row
        wild.append(t)
    for t in wild:
        assert call(t) == MCVC_ERR_INVALID
    assert call(None) == MCVC_ERR_INVALID and call(good_tiles, x_ptr=None) == MCVC_ERR_INVALID and call(good_tiles, table_ptr=None) == MCVC_ERR_INVALID
    assert call(good_tiles, y_ptr=None) == MCVC_ERR_INVALID and call(good_tiles, n_tiles=0) == MCVC_ERR_INVALID
    assert call(good_tiles, u=4, d=2) == MCVC_ERR_INVALID and call(good_tiles, u=641, d=2) == MCVC_ERR_INVALID and call(good_tiles, u=3, d=3) == MCVC_ERR_INVALID
    assert call(good_tiles, n_out=total - 1) == MCVC_ERR_INVALID and call(good_tiles, n_in=4999) == MCVC_ERR_INVALID
    assert call(good_tiles, y_ptr=ctypes.c_void_p(out.data_ptr() + 2)) == MCVC_ERR_INVALID                 # misaligned
    assert call(good_tiles, table_ptr=ctypes.c_void_p(table.data_ptr() + 4)) == MCVC_ERR_INVALID
    pageable = np.ascontiguousarray(good_tiles.numpy().copy())            # a work list the device could not read: refused, not followed
    assert L.mcvc_resample_run(_hip.ptr(xt), 5000, pageable.ctypes.data, nt.value, _hip.ptr(table), up, down, _hip.ptr(out), total, _hip.stream()) == MCVC_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                       # nothing was launched
    assert call(good_tiles) == 0                                          # and the untouched arguments do work
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), run(rs, [x], up, down)[0])


# ---- 4. the front-end path -------------------------------------------------------------------------------------------------------------
def test_bank_at_rates_is_resampler_then_bank(rs, golden_dir):
    """Plumbing only (the arithmetic is covered above): the mels of a 16 kHz, a 48 kHz and the 22050 Hz version of one recording equal
    Audio2Mel.bank applied to the Resampler's own output, bit for bit, and the 22050 Hz entry equals bank([read_wav(...)])."""
    fft = Audio2Mel()
    x = read_wav(os.path.join(golden_dir, "audio", "real_VCC2SF3.wav"))
    x16 = signal.resample_poly(x.astype(np.float64), 320, 441).astype(np.float32)
    x48 = signal.resample_poly(x.astype(np.float64), 320, 147).astype(np.float32)
    got = fft.bank_at_rates([x16, x, x48, x16[:9000]], [16000, 22050, 48000, 16000])
    back16, back16s = rs.bank([x16, x16[:9000]], 16000, 22050, to_host=True)
    (back48,) = rs.bank([x48], 48000, 22050, to_host=True)
    want = fft.bank([back16, x, back48, back16s])
    assert len(got) == 4
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and np.array_equal(g, w)
    assert np.array_equal(got[1], fft.bank([x])[0])
    assert got[0].shape == (80, num_frames(ck.out_len(x16.size, 441, 320)))
    with pytest.raises(ValueError, match="waveforms but"):
        fft.bank_at_rates([x], [16000, 22050])


# ---- 5. the command lines --------------------------------------------------------------------------------------------------------------
def _clips_16k(root, golden_dir):
    """<root>/SPK/{a,b}.wav: the two committed recordings brought to 16 kHz with scipy, as int16 PCM -> what the files hold, as float32."""
    os.makedirs(os.path.join(root, "SPK"))
    waves = []
    for name, out in (("real_VCC2SF3.wav", "a.wav"), ("real_VCC2TF1.wav", "b.wav")):
        rate, pcm = wavfile.read(os.path.join(golden_dir, "audio", name))
        assert rate == 22050 and pcm.dtype == np.int16
        y = np.clip(np.round(signal.resample_poly(pcm.astype(np.float64), 320, 441)), -32768, 32767).astype(np.int16)
        wavfile.write(os.path.join(root, "SPK", out), 16000, y)
        waves.append((y.astype(np.float64) / 32768.0).astype(np.float32))
    return waves


def test_preprocess_cli_gpu_resample(tmp_path, golden_dir, rs):
    waves = _clips_16k(str(tmp_path / "wavs"), golden_dir)
    preprocess_vcc2018.main(["--data_directory", str(tmp_path / "wavs"), "--preprocessed_data_directory", str(tmp_path / "out"), "--speaker_ids", "SPK",
                             "--gpu_resample"])
    mels, mean, std = load_speaker(str(tmp_path / "out"), "SPK")
    frames = [num_frames(ck.out_len(w.size, 441, 320)) for w in waves]
    assert len(mels) == 2 and [m.shape for m in mels] == [(80, f) for f in frames] and mean.shape == (80, 1) and std.shape == (80, 1)
    # the pickle is the module path's result: resampler, front-end, the writer's own standardisation
    want, wmean, wstd = preprocess_vcc2018.normalize_mels(Audio2Mel().bank(rs.bank(waves, 16000, 22050, to_host=True)))
    assert np.array_equal(mean, wmean) and np.array_equal(std, wstd) and all(np.array_equal(m, w) for m, w in zip(mels, want))


def test_inference_cli_gpu_resample_and_out_sample_rate(tmp_path, golden_dir):
    from mask_cyclegan_vc import test as test_cli
    _clips_16k(str(tmp_path / "clips"), golden_dir)
    data = str(tmp_path / "data")
    rng = np.random.RandomState(4)
    for spk in ("SPKA", "SPKB"):
        os.makedirs(os.path.join(data, spk))
        with open(os.path.join(data, spk, "%s_normalized.pickle" % spk), "wb") as fh:
            pickle.dump([rng.randn(80, 64).astype(np.float32)], fh)
        np.savez(os.path.join(data, spk, "%s_norm_stat.npz" % spk), mean=(-2.0 + rng.randn(80, 1)).astype(np.float32), std=(1 + rng.rand(80, 1)).astype(np.float32))
    ck_dir = tmp_path / "ckpts"
    ck_dir.mkdir()
    torch.save({"ckpt_info": {"epoch": 1}, "model_class": "Generator", "model_state": orc.filler_params("G", 11), "optimizer": None,
                "lr_scheduler": None}, str(ck_dir / "00001_generator_A2B.pth.tar"))
    common = ["--save_dir", str(tmp_path / "res"), "--preprocessed_data_dir", data, "--speaker_A_id", "SPKA", "--speaker_B_id", "SPKB",
              "--ckpt_dir", str(ck_dir), "--load_epoch", "1", "--model_name", "generator_A2B", "--wav_dir", str(tmp_path / "clips"), "--gpu_resample",
              "--griffin_lim", "2"]
    test_cli.main(["--name", "at22k"] + common)                           # the decoder's own 22050 Hz output
    test_cli.main(["--name", "at16k", "--out_sample_rate", "16000"] + common)
    names = sorted("%d-%s_SPKA_to_SPKB.wav" % (i, k) for i in (0, 1) for k in ("converted", "original"))
    d22, d16 = (str(tmp_path / "res" / n / "converted_audio") for n in ("at22k", "at16k"))
    assert sorted(os.listdir(d22)) == names == sorted(os.listdir(d16))
    worst = 0.0
    for n in names:
        r22, w22 = wavfile.read(os.path.join(d22, n))
        r16, w16 = wavfile.read(os.path.join(d16, n))
        assert r22 == 22050 and r16 == 16000 and w22.dtype == w16.dtype == np.float32 and w22.size % 256 == 0
        assert w16.shape == (-(-w22.size * 320 // 441),)                  # ceil(256 T 320 / 441)
        worst = max(worst, ck.check("--out_sample_rate 16000 %s" % n, w16, w22, 320, 441))
    record("cli 320/441", worst)
