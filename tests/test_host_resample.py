"""CPU-only checks of the resampler's host side (data_preprocessing/resample.py, the mcvc_resample_* C ABI, the new command-line flags) and
of the float64 checker itself (tests/resample_checker.py) against scipy.  No kernel is launched here."""
import ctypes
import os

import numpy as np
import pytest
from scipy import signal
from scipy.io import wavfile

import resample_checker as ck
from args.cycleGAN_test_arg_parser import CycleGANTestArgParser
from data_preprocessing import audio2mel, preprocess_vcc2018, resample
from mask_cyclegan_vc import _hip

MCVC_ERR_INVALID, MCVC_ERR_WORKSPACE = 1001, 1002
SYMBOLS = ("mcvc_resample_max_factor", "mcvc_resample_tile_samples", "mcvc_resample_out_samples", "mcvc_resample_table_floats",
           "mcvc_resample_pack", "mcvc_resample_plan", "mcvc_resample_run")
# rates, (up, down), input lengths: the cases of the issue
SCIPY_CASES = [(16000, 22050, 441, 320, (1000,)), (48000, 22050, 147, 320, (3001, 1)), (44100, 22050, 1, 2, (777,)), (22050, 16000, 320, 441, (1500,)),
               (22050, 48000, 320, 147, (400,)), (24000, 22050, 147, 160, (1234,)), (8000, 22050, 441, 160, (50,)), (22050, 44100, 2, 1, (3,))]
TAP_PAIRS = [(441, 320), (147, 320), (1, 2), (2, 1), (320, 441), (147, 640)]


@pytest.mark.parametrize("r_in,r_out,up,down,lengths", SCIPY_CASES)
def test_checker_is_scipy_resample_poly(r_in, r_out, up, down, lengths):
    assert resample.ratio(r_in, r_out) == (up, down)
    for n in lengths:
        x = np.random.RandomState(n).randn(n)
        want = signal.resample_poly(x, up, down)
        got, mag, terms = ck.resample(x, up, down)
        assert got.shape == want.shape == (ck.out_len(n, up, down),) == (resample.out_samples(n, up, down),)
        err = float(np.abs(got - want).max())
        print("%d -> %d Hz, n_in %d: |checker - scipy| <= %.2e, terms %d .. %d" % (r_in, r_out, n, err, terms.min(), terms.max()))
        assert err <= 1e-12
        assert (mag >= np.abs(got) - 1e-12).all() and terms.max() <= 20 * max(up, down) // up + 1


@pytest.mark.parametrize("up,down", TAP_PAIRS)
def test_taps_are_scipys_firwin(up, down):
    m = max(up, down)
    want = up * signal.firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0))
    for name, h in (("resample_taps", resample.resample_taps(up, down)), ("checker", ck.taps(up, down))):
        assert h.dtype == np.float64 and h.shape == want.shape
        assert np.abs(h - want).max() <= 1e-14 * np.abs(want).max(), name
    assert abs(resample.resample_taps(up, down).sum() - up) <= 1e-12 * up


def test_resample_module_does_not_import_scipy():
    with open(resample.__file__.replace(".pyc", ".py")) as fh:
        text = fh.read()
    assert "import scipy" not in text and "from scipy" not in text


def test_symbols_are_declared_exported_and_bound():
    L = _hip.lib()
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcvc.h")) as fh:
        header = fh.read()
    for s in SYMBOLS:
        assert s + "(" in header and s in _hip._SIGS and s in _hip.EXPORTED_SYMBOLS and hasattr(L, s), s
    assert "#define MCVC_ABI_VERSION 3 " in header and L.mcvc_version() == 3
    assert L.mcvc_resample_max_factor() >= 640 and L.mcvc_resample_max_factor() == resample.MAX_FACTOR
    assert L.mcvc_resample_tile_samples() >= 64


@pytest.mark.parametrize("up,down", TAP_PAIRS + [(320, 147), (640, 441), (1, 640), (640, 1)])
def test_pack_places_every_tap_exactly_once(up, down):
    L = _hip.lib()
    m = max(up, down)
    n_taps = 20 * m + 1
    h = np.arange(1, n_taps + 1, dtype=np.float32)                      # every tap its own non-zero value, exact in float32
    nf = L.mcvc_resample_table_floats(up, down)
    J = -(-n_taps // up)
    assert nf >= up * J and nf % 4 == 0
    table = np.full(nf + 8, -7.0, dtype=np.float32)
    assert L.mcvc_resample_pack(h.ctypes.data, n_taps, up, down, table.ctypes.data) == 0
    assert (table[nf:] == -7.0).all()                                   # nothing past the size it reported
    body = table[:nf]
    assert np.array_equal(np.sort(body[body != 0]), h)                  # each tap once, everything else zero
    pitch = J | 1
    assert nf == -(-(up * pitch) // 4) * 4
    for n in (0, 1, up - 1, up, n_taps // 2, n_taps - 1):
        assert body[(n % up) * pitch + n // up] == h[n], n              # P[r][j] = h[r + j up] at pitch J | 1
    for bad in (n_taps - 1, n_taps + 1, 0):
        before = table.copy()
        assert L.mcvc_resample_pack(h.ctypes.data, bad, up, down, table.ctypes.data) == MCVC_ERR_INVALID
        assert np.array_equal(table, before)
    assert L.mcvc_resample_pack(None, n_taps, up, down, table.ctypes.data) == MCVC_ERR_INVALID
    assert L.mcvc_resample_pack(h.ctypes.data, n_taps, up, down, None) == MCVC_ERR_INVALID


def test_table_floats_and_out_samples():
    L = _hip.lib()
    for up, down in TAP_PAIRS + [(320, 147)]:
        for n in (1, 2, 319, 320, 321, 57344):
            assert L.mcvc_resample_out_samples(n, up, down) == -(-n * up // down) == ck.out_len(n, up, down), (n, up, down)
    assert L.mcvc_resample_out_samples(2 ** 40, 441, 320) == -(-2 ** 40 * 441 // 320)
    for n, up, down in ((0, 1, 2), (-1, 1, 2), (5, 0, 2), (5, 2, 0), (5, 641, 2), (5, 2, 641), (5, -1, 2)):
        assert L.mcvc_resample_out_samples(n, up, down) == 0
    assert L.mcvc_resample_table_floats(641, 2) == 0 and L.mcvc_resample_table_floats(0, 2) == 0


def _plan(offs, up, down, max_tiles=None):
    L = _hip.lib()
    offs = np.asarray(offs, dtype=np.int32)
    n = offs.size - 1
    out_offs = np.full(n + 1, -1, dtype=np.int32)
    nt = ctypes.c_int(-1)
    rc = L.mcvc_resample_plan(offs.ctypes.data, n, up, down, out_offs.ctypes.data, None, 0, ctypes.byref(nt))
    if rc != 0:
        return rc, None, None
    tiles = np.full((nt.value if max_tiles is None else max_tiles, 8), -1, dtype=np.int32)
    nt2 = ctypes.c_int(-1)
    rc = L.mcvc_resample_plan(offs.ctypes.data, n, up, down, out_offs.ctypes.data, tiles.ctypes.data, tiles.shape[0], ctypes.byref(nt2))
    assert nt2.value == nt.value
    return rc, out_offs, tiles


@pytest.mark.parametrize("up,down", [(441, 320), (147, 320), (1, 2), (320, 147), (2, 1), (147, 640), (1, 640), (640, 1), (639, 640)])
def test_plan_covers_every_output_once(up, down):
    L = _hip.lib()
    TILE = L.mcvc_resample_tile_samples()
    lens = [1, 2, 5000, 319, 320, 321, 20001, 3 * TILE, 7]
    offs = np.concatenate([[0], np.cumsum(lens)])
    rc, out_offs, tiles = _plan(offs, up, down)
    assert rc == 0
    n_out = [ck.out_len(n, up, down) for n in lens]
    assert np.array_equal(out_offs, np.concatenate([[0], np.cumsum(n_out)]))
    cover = np.zeros(out_offs[-1], dtype=np.int32)
    half = 10 * max(up, down)
    for in_off, n_in, out0, n, q0, r0, z0, z1 in tiles.tolist():
        u = int(np.searchsorted(offs, in_off, side="right")) - 1
        assert in_off == offs[u] and n_in == lens[u] and 1 <= n <= TILE and z0 == 0 and z1 == 0
        assert out_offs[u] <= out0 and out0 + n <= out_offs[u + 1]        # a row never crosses an utterance
        cover[out0:out0 + n] += 1
        c = (out0 - int(out_offs[u])) * down + half
        assert (q0, r0) == divmod(c, up)
    assert (cover == 1).all()
    # the size-then-fill protocol: a short list is refused, the count is still reported
    if tiles.shape[0] > 1:
        rc, _, short = _plan(offs, up, down, max_tiles=tiles.shape[0] - 1)
        assert rc == MCVC_ERR_WORKSPACE and np.array_equal(short, tiles[:-1])


def test_plan_refusals():
    L = _hip.lib()
    good = [0, 100, 300]
    assert _plan(good, 441, 320)[0] == 0
    for offs, up, down, why in (([0, 100, 100], 441, 320, "an empty utterance"), ([0, 100, 50], 441, 320, "offsets that fall"),
                                ([-1, 100, 300], 441, 320, "a negative offset"), (good, 3, 3, "up == down"), (good, 1, 1, "up == down"),
                                (good, 4, 2, "gcd 2"), (good, 641, 2, "factor over the maximum"), (good, 3, 641, "factor over the maximum"),
                                (good, 0, 2, "zero factor"), ([0, 2 ** 30], 2, 1, "2^31 output samples")):
        assert _plan(offs, up, down)[0] == MCVC_ERR_INVALID, why
    oo = np.zeros(3, dtype=np.int32)
    nt = ctypes.c_int(0)
    big = np.array([0, 2 ** 30 - 1], dtype=np.int32)                    # 2^31 - 2 output samples: accepted (sized only, tiles = NULL)
    assert L.mcvc_resample_plan(big.ctypes.data, 1, 2, 1, oo.ctypes.data, None, 0, ctypes.byref(nt)) == 0
    assert oo[1] == 2 ** 31 - 2 and nt.value == -(-(2 ** 31 - 2) // L.mcvc_resample_tile_samples())
    offs = np.array(good, dtype=np.int32)
    assert L.mcvc_resample_plan(offs.ctypes.data, 0, 441, 320, oo.ctypes.data, None, 0, ctypes.byref(nt)) == MCVC_ERR_INVALID
    assert L.mcvc_resample_plan(None, 2, 441, 320, oo.ctypes.data, None, 0, ctypes.byref(nt)) == MCVC_ERR_INVALID
    assert L.mcvc_resample_plan(offs.ctypes.data, 2, 441, 320, None, None, 0, ctypes.byref(nt)) == MCVC_ERR_INVALID
    assert L.mcvc_resample_plan(offs.ctypes.data, 2, 441, 320, oo.ctypes.data, None, 0, None) == MCVC_ERR_INVALID


def test_plan_indices_beyond_32_bits():
    """10^7 input samples at 441/320: the last outputs have k down > 2^32; (q, r) of the last row equal Python's integers."""
    up, down, n_in = 441, 320, 10 ** 7
    rc, out_offs, tiles = _plan([0, 5, 5 + n_in], up, down)
    assert rc == 0
    n_out = ck.out_len(n_in, up, down)
    assert out_offs.tolist() == [0, 7, 7 + n_out]
    in_off, n_len, out0, n, q0, r0 = tiles[-1, :6].tolist()
    k = out0 - 7
    assert k * down > 2 ** 32 and in_off == 5 and n_len == n_in and out0 + n == 7 + n_out
    assert (q0, r0) == divmod(k * down + 10 * up, up)


def test_new_flags_of_the_parsers(tmp_path, capsys):
    base = ["--save_dir", str(tmp_path), "--name", "r", "--ckpt_dir", str(tmp_path), "--load_epoch", "1"]
    p = CycleGANTestArgParser().parser                                  # (the bare parser: the wrapper's parse_args creates run directories)
    d = p.parse_args([])
    assert d.out_sample_rate is None and d.gpu_resample is False
    with pytest.raises(SystemExit):
        CycleGANTestArgParser().parse_args(base + ["--out_sample_rate", "16000"])
    assert "--vocoder_ckpt or --griffin_lim" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        CycleGANTestArgParser().parse_args(base + ["--gpu_resample"])
    assert "--wav_dir" in capsys.readouterr().err
    a = CycleGANTestArgParser().parse_args(base + ["--griffin_lim", "2", "--out_sample_rate", "16000", "--wav_dir", "w", "--gpu_resample"])
    assert a.out_sample_rate == 16000 and a.gpu_resample and a.sample_rate == 22050
    a = CycleGANTestArgParser().parse_args(base + ["--vocoder_ckpt", "melgan.pt", "--out_sample_rate", "48000"])
    assert a.out_sample_rate == 48000 and not a.gpu_resample
    ap = preprocess_vcc2018.build_parser()
    assert ap.parse_args(["--data_directory", "w", "--speaker_ids", "A"]).gpu_resample is False
    assert ap.parse_args(["--data_directory", "w", "--speaker_ids", "A", "--gpu_resample"]).gpu_resample is True
    with pytest.raises(SystemExit):
        preprocess_vcc2018.main(["--mel_directory", "m", "--speaker_ids", "A", "--gpu_resample"])
    assert "--data_directory" in capsys.readouterr().err
    for text in (p.format_help(), ap.format_help()):
        assert "--gpu_resample" in text


def test_read_wav_native_plus_host_resampling_is_read_wav(tmp_path):
    rs = np.random.RandomState(3)
    pcm = (8000 * rs.randn(4000, 2)).astype(np.int16)                   # 16 kHz stereo
    path = str(tmp_path / "x16k.wav")
    wavfile.write(path, 16000, pcm)
    rate, x = audio2mel.read_wav_native(path)
    assert rate == 16000 and isinstance(rate, int) and x.dtype == np.float32 and x.shape == (4000,)
    assert np.array_equal(x, (pcm.astype(np.float64) / 32768.0).astype(np.float32).mean(axis=1, dtype=np.float32))
    want = audio2mel.read_wav(path)
    got = np.ascontiguousarray(signal.resample_poly(x.astype(np.float64), 441, 320), dtype=np.float32)
    assert want.shape == (ck.out_len(4000, 441, 320),) and np.array_equal(got, want)
    path22 = str(tmp_path / "x22k.wav")
    wavfile.write(path22, 22050, pcm[:, 0])
    rate, x = audio2mel.read_wav_native(path22)
    assert rate == 22050 and np.array_equal(x, audio2mel.read_wav(path22))


def test_cpu_tensors_and_large_factors_are_refused():
    with pytest.raises(ValueError, match="limit of 640"):
        resample._check_factors(641, 2)
    assert resample.ratio(22050, 96000) == (640, 147) and resample.ratio(44100, 44100) == (1, 1)
    with pytest.raises(ValueError, match="positive"):
        resample.ratio(0, 22050)
