"""CPU-only checks of the modulation-spectrum host side (mask_cyclegan_vc/metrics.py, the mcvc_ms_* C ABI, the evaluate parser) and of the
float64 checker itself (tests/ms_checker.py) against facts that need no kernel.  No kernel is launched here: every ABI call below is one
the library refuses before it touches a pointer."""
import math

import numpy as np
import pytest

import ms_checker as ck
from args.evaluate_arg_parser import EvaluateArgParser
from mask_cyclegan_vc import _hip, metrics

MCVC_ERR_INVALID = 1001
MS_SYMBOLS = ("mcvc_ms_max_fft", "mcvc_ms_launches", "mcvc_ms_table_init", "mcvc_ms_power", "mcvc_ms_mean_log", "mcvc_ms_distance")


# ---- the checker against facts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,b", [(1024, 1), (1024, 37), (1024, 512), (4096, 1000), (4096, 2048)])
def test_checker_cosine_at_an_integer_bin(n_fft, b):
    """cos(2 pi b t / T) over T = n_fft frames has X[b] = T / 2 (T at Nyquist) and nothing elsewhere: P[b] = T / 4 (T at Nyquist)."""
    T = n_fft
    c = np.cos(2.0 * np.pi * b * np.arange(T) / T)[None, :]
    P, mean, var = ck.power(c, n_fft)
    peak = T if b == n_fft // 2 else T / 4.0
    assert abs(P[0, b - 1] - peak) <= 1e-9 * peak
    rest = np.delete(P[0], b - 1)
    assert rest.max() < 1e-20 * T
    assert abs(mean[0]) < 1e-12 and abs(var[0] - (1.0 if b == n_fft // 2 else 0.5)) < 1e-12


@pytest.mark.parametrize("n_fft,T", [(1024, 1), (1024, 2), (1024, 65), (1024, 1024), (2048, 700), (4096, 130)])
def test_checker_parseval(n_fft, T):
    """2 sum_{f = 1}^{n_fft / 2 - 1} P_f + P_{n_fft / 2} = n_fft var: the zero-padded signal's energy, bin 0 being empty."""
    c = ck.trajectory(np.random.RandomState(T), 3, T)
    P, _, var = ck.power(c, n_fft)
    lhs = 2.0 * P[:, :-1].sum(axis=1) + P[:, -1]
    assert np.abs(lhs - n_fft * var).max() <= 1e-11 * max(1.0, float((n_fft * var).max()))


def test_checker_degenerate_rows_sit_on_the_floor():
    for c in (np.full((2, 40), 0.1, dtype=np.float32), np.float32([[3.0], [-1.5]]), np.zeros((1, 7), dtype=np.float32)):
        P, mean, var = ck.power(c, 1024)
        assert (var == 0.0).all() and (P == 0.0).all() and np.array_equal(mean, c[:, 0].astype(np.float64))
        lms, lgv = ck.tables([c], 1024)
        want = 10.0 * math.log10(ck.FLOOR)
        assert np.abs(lms - want).max() < 1e-12 and np.abs(lgv - want).max() < 1e-12 and abs(want + 100.0) < 1e-12


def test_checker_distance_of_a_set_with_itself_and_with_a_scaled_copy():
    rs = np.random.RandomState(3)
    A = [ck.trajectory(rs, 5, T).astype(np.float64) for T in (63, 130, 200)]
    res = ck.msd(A, A, 1024)
    assert res["msd"] == 0.0 and res["gvd"] == 0.0 and (res["msd_per_dim"] == 0.0).all()
    for g in (0.5, 3.0):
        shift = 20.0 * math.log10(g)
        res = ck.msd([g * a for a in A], A, 1024)
        assert np.abs(res["lms_a"] - res["lms_b"] - shift).max() < 1e-9 and np.abs(res["lgv_a"] - res["lgv_b"] - shift).max() < 1e-9
        assert abs(res["msd"] - abs(shift)) < 1e-9 and abs(res["gvd"] - abs(shift)) < 1e-9 and np.abs(res["msd_per_dim"] - abs(shift)).max() < 1e-9
    # sets of different sizes, a band limit
    B = [ck.trajectory(rs, 5, T, noise=0.1) for T in (80, 90)]
    res = ck.msd(A, B, 1024, max_hz=10.0)
    assert res["n_bins_used"] == 118 and res["msd"] > 0.0 and res["msd_per_dim"].shape == (5,)
    assert abs(res["msd"] - math.sqrt(float((res["msd_per_dim"] ** 2).mean()))) < 1e-12


def test_bin_selection_matches_the_checker():
    for n_fft in ck.FFTS:
        assert metrics.ms_bins(n_fft) == (n_fft // 2, ck.FRAME_RATE / 2.0)
        for hz in (0.1, 1.0, 10.0, 43.0, ck.FRAME_RATE / 2.0):
            assert metrics.ms_bins(n_fft, hz) == (ck.bins_used(n_fft, hz), hz), (n_fft, hz)
    for bad in (0.0, 0.01, -3.0, 50.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_hz"):
            metrics.ms_bins(1024, bad)
    for bad in (512, 1000, 8192, 0, 1024.5):
        with pytest.raises(ValueError, match="n_fft"):
            metrics.ms_bins(bad)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_bound():
    L = _hip.lib()
    for name in MS_SYMBOLS:
        assert name in _hip.EXPORTED_SYMBOLS and getattr(L, name).argtypes is not None
    assert L.mcvc_version() == 3
    assert L.mcvc_ms_max_fft() == 4096 == L.mcvc_dtw_max_frames()
    assert L.mcvc_ms_launches() == 8


@pytest.mark.parametrize("n_fft", ck.FFTS)
def test_table_is_the_cosine_rounded_once(n_fft):
    host = metrics.host_ms_table(n_fft)
    want = np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    assert host.dtype == np.float32 and host.shape == (n_fft,)
    assert np.abs(host.astype(np.float64) - want).max() <= 2.0 ** -25 * 1.01                 # half an ulp of a number below 1 (two libraries' cos: 1e-16)
    assert np.count_nonzero(host != want.astype(np.float32)) <= 1 + n_fft // 100
    assert host[0] == 1.0 and host[n_fft // 2] == -1.0 and abs(host[n_fft // 4]) < 1e-15


def test_table_init_refusals():
    L = _hip.lib()
    buf = np.zeros(4096 + 4, dtype=np.float32)
    for bad in (0, 512, 1000, 8192, -1024):
        assert L.mcvc_ms_table_init(bad, buf.ctypes.data) == MCVC_ERR_INVALID
        with pytest.raises(ValueError):
            metrics.host_ms_table(bad)
    assert L.mcvc_ms_table_init(1024, None) == MCVC_ERR_INVALID
    assert L.mcvc_ms_table_init(1024, buf.ctypes.data + 2) == MCVC_ERR_INVALID


def aligned(n_floats):
    """A host buffer whose address is a multiple of 64: a stand-in for a device pointer in a call that is refused before it is used."""
    raw = np.zeros(n_floats + 16, dtype=np.float32)
    shift = (-raw.ctypes.data % 64) // 4
    return raw[shift:shift + n_floats]


def test_power_refusals():
    L = _hip.lib()
    K, n_fft = 4, 1024
    offs = np.array([0, 10, 30], dtype=np.int32)
    bufs = {name: aligned(64) for name in ("cep", "offs_dev", "table", "power", "mean", "var")}

    def call(K=K, n_frames=30, n_utts=2, offs=offs, n_fft=n_fft, **ptrs):
        p = {name: b.ctypes.data for name, b in bufs.items()}
        p["offs_host"] = None if offs is None else offs.ctypes.data
        p.update(ptrs)
        return L.mcvc_ms_power(p["cep"], n_frames, K, p["offs_dev"], n_utts, p["offs_host"], n_fft, p["table"], p["power"], p["mean"], p["var"], None)

    for name in bufs:
        assert call(**{name: None}) == MCVC_ERR_INVALID, name
        assert call(**{name: bufs[name].ctypes.data + 2}) == MCVC_ERR_INVALID, name
    assert call(table=bufs["table"].ctypes.data + 4) == MCVC_ERR_INVALID                    # the table is read 16 bytes at a time
    assert call(offs=None) == MCVC_ERR_INVALID
    for bad in (0, 81, -1):
        assert call(K=bad) == MCVC_ERR_INVALID
    for bad in (0, 512, 1000, 8192):
        assert call(n_fft=bad) == MCVC_ERR_INVALID
    assert call(n_utts=0) == MCVC_ERR_INVALID
    for bad in ([1, 10, 30], [0, 10, 29], [0, 10, 31], [0, 30, 30], [0, 31, 30], [0, -1, 30]):
        assert call(offs=np.array(bad, dtype=np.int32)) == MCVC_ERR_INVALID, bad
    assert call(n_frames=0, n_utts=1, offs=np.array([0, 0], dtype=np.int32)) == MCVC_ERR_INVALID
    for n_fft_ in ck.FFTS:                                                                  # one frame more than the transform holds
        assert call(n_frames=n_fft_ + 11, offs=np.array([0, 10, n_fft_ + 11], dtype=np.int32), n_fft=n_fft_) == MCVC_ERR_INVALID


def test_mean_log_and_distance_refusals():
    L = _hip.lib()
    a, b, out, tot = aligned(64), aligned(64), aligned(64), aligned(4)
    pa, pb, po, pt = a.ctypes.data, b.ctypes.data, out.ctypes.data, tot.ctypes.data
    for v, o in ((None, po), (pa, None), (pa + 1, po), (pa, po + 2)):
        assert L.mcvc_ms_mean_log(v, 2, 8, 1e-10, o, None) == MCVC_ERR_INVALID
    for n in (0, -1):
        assert L.mcvc_ms_mean_log(pa, n, 8, 1e-10, po, None) == MCVC_ERR_INVALID
    assert L.mcvc_ms_mean_log(pa, 2, 0, 1e-10, po, None) == MCVC_ERR_INVALID
    for floor in (0.0, -1e-10, float("inf"), float("nan")):
        assert L.mcvc_ms_mean_log(pa, 2, 8, floor, po, None) == MCVC_ERR_INVALID
    for args in ((None, pb, po, pt), (pa, None, po, pt), (pa, pb, None, pt), (pa, pb, po, None), (pa + 2, pb, po, pt), (pa, pb + 1, po, pt),
                 (pa, pb, po + 2, pt), (pa, pb, po, pt + 2)):
        assert L.mcvc_ms_distance(args[0], args[1], 2, 8, 8, args[2], args[3], None) == MCVC_ERR_INVALID
    for K in (0, 81):
        assert L.mcvc_ms_distance(pa, pb, K, 8, 8, po, pt, None) == MCVC_ERR_INVALID
    for n_bins, n_used in ((8, 0), (8, 9), (8, -1), (0, 0), (2049, 1)):
        assert L.mcvc_ms_distance(pa, pb, 2, n_bins, n_used, po, pt, None) == MCVC_ERR_INVALID


# ---- the parser --------------------------------------------------------------------------------------------------------------------------
BASE = ["--target_wav_dir", "x"]


def test_parser_defaults_are_unchanged():
    args = EvaluateArgParser().parse_args(BASE)
    assert vars(args) == dict(name="debug", save_dir="/home/results/", converted_dir=None, preprocessed_data_dir="vcc2018_training_preprocessed/",
                              target_speaker_id=None, target_wav_dir="x", source_speaker_id=None, n_cep=24, f0=False, converted_audio_dir=None,
                              f0_min=60.0, f0_max=500.0, f0_threshold=0.15, msd=False, msd_n_fft=4096, msd_max_hz=None, no_mcd=False)


def test_parser_accepts_the_msd_flags():
    args = EvaluateArgParser().parse_args(BASE + ["--msd"])
    assert args.msd and not args.no_mcd and args.msd_n_fft == 4096 and args.msd_max_hz is None
    args = EvaluateArgParser().parse_args(BASE + ["--msd", "--no_mcd", "--msd_n_fft", "1024", "--msd_max_hz", "10"])
    assert args.msd and args.no_mcd and args.msd_n_fft == 1024 and args.msd_max_hz == 10.0
    assert EvaluateArgParser().parse_args(BASE + ["--msd", "--f0"]).f0


@pytest.mark.parametrize("extra,word", [(["--msd", "--msd_n_fft", "512"], "msd_n_fft"), (["--no_mcd"], "--msd"), (["--msd", "--no_mcd", "--f0"], "--f0"),
                                        (["--msd", "--msd_max_hz", "0"], "no bin"), (["--msd", "--msd_max_hz", "50"], "Nyquist")])
def test_parser_refusals(extra, word, capsys):
    with pytest.raises(SystemExit):
        EvaluateArgParser().parse_args(BASE + extra)
    assert word in capsys.readouterr().err
