"""CPU-only checks of the pitch tracker's host side (mask_cyclegan_vc/pitch.py, the mcvc_f0_* C ABI, the evaluate parser's --f0 flags) and of
the float64 checker itself (tests/f0_checker.py).  No kernel is launched here."""
import numpy as np
import pytest
import torch

import f0_checker as ck
from args.evaluate_arg_parser import EvaluateArgParser
from mask_cyclegan_vc import _hip, metrics, pitch

MCVC_ERR_INVALID = 1001
F0_SYMBOLS = ("mcvc_f0_max_lag", "mcvc_f0_launches", "mcvc_f0_track", "mcvc_f0_stats")


def interior(n_samples, tau_max):
    """Frames whose whole window buf[0 .. W + tau_max) lies inside the signal."""
    return [t for t in range(ck.frames_of(n_samples))
            if ck.HOP * t + ck.HOP // 2 - (ck.W + tau_max) // 2 >= 0 and ck.HOP * t + ck.HOP // 2 - (ck.W + tau_max) // 2 + ck.W + tau_max <= n_samples]


# ---- the checker against facts that need no kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", (0.0, 0.37))
def test_checker_silence_and_dc_are_unvoiced(value):
    x = np.full(4096, value)
    f0, ap, dp, tau = ck.track(x)
    inner = interior(x.size, 367)
    assert inner and (dp[:, inner] == 1.0).all()
    assert (f0[inner] == 0.0).all() and (ap[inner] == 1.0).all() and (tau[inner] == 0).all()
    if value == 0.0:                                                  # (a constant meets the zero padding at the edges: only silence is flat there)
        assert (dp == 1.0).all() and (f0 == 0.0).all() and (ap == 1.0).all()


def test_checker_pulse_train_of_period_100():
    """+1 at n = 0 mod 100, -1 at n = 50 mod 100: d(100) is exactly 0 on interior frames, the pick lands on tau = 100 with aperiodicity 0.
    The parabola runs on d', whose running mean is not symmetric about the dip (for a flat d, d'(99) = 1 against d'(101) = 1.01), so the
    offset is about a hundredth of a lag and not 0: f0 = 220.5 Hz within 2e-4."""
    x = np.zeros(8192)
    x[0::100] = 1.0
    x[50::100] = -1.0
    f0, ap, dp, tau = ck.track(x)
    inner = interior(x.size, 367)
    assert len(inner) >= 20
    for t in inner:
        assert ck.difference(x, t, 367)[100] == 0.0 and dp[100, t] == 0.0
        voiced, tt, off, f, a = ck.pick(dp[:, t], 45, 367, 0.15)
        assert voiced and tt == 100 and tau[t] == 100 and a == 0.0 and ap[t] == 0.0
        assert abs(off) <= 2e-2 and abs(f - 220.5) <= 2e-4 * 220.5 and f == f0[t]


def test_checker_pick_on_a_hand_written_array():
    #      tau:  0    1    2    3     4     5     6    7    8    9
    dp = [1.0, 1.0, 0.9, 0.5, 0.14, 0.10, 0.12, 0.3, 0.1, 0.05]
    # the threshold stops the scan at 4, the descent walks to 5 and stops at the strict comparison with 0.12
    voiced, tau, off, f0, ap = ck.pick(dp, 2, 9, 0.15)
    want = 0.5 * (0.14 - 0.12) / ((0.14 - 0.10) + (0.12 - 0.10))
    assert voiced and tau == 5 and ap == 0.10 and abs(off - want) <= 1e-15 and f0 == ck.SR / (5 + off)
    assert ck.comparisons(dp, 2, 9, 0.15) == [(0.9, 0.15), (0.5, 0.15), (0.14, 0.15), (0.10, 0.14), (0.12, 0.10)]
    # a lower threshold passes the first dip: the scan reaches 8, descends to tau_max = 9, and there off = 0
    voiced, tau, off, f0, ap = ck.pick(dp, 2, 9, 0.101)
    assert voiced and tau == 5                                       # 0.10 < 0.101: still the first dip
    voiced, tau, off, f0, ap = ck.pick(dp, 2, 9, 0.10)               # strict: 0.10 is not under 0.10, 8 is not either, 9 is
    assert voiced and tau == 9 and off == 0.0 and f0 == ck.SR / 9 and ap == 0.05
    voiced, tau, off, f0, ap = ck.pick(dp, 7, 9, 0.15)               # starts beyond the first dip: 8, then the descent to the edge
    assert voiced and tau == 9 and off == 0.0
    # nothing under the threshold: unvoiced, aperiodicity = the minimum over the range only
    voiced, tau, off, f0, ap = ck.pick(dp, 2, 7, 0.05)
    assert (voiced, tau, off, f0, ap) == (False, 0, 0.0, 0.0, 0.10)
    assert len(ck.comparisons(dp, 2, 7, 0.05)) == 6
    # den == 0 (a flat triple) and den < 0 (a < b at the first lag scanned): off = 0
    assert ck.pick([1.0, 1.0, 0.1, 0.1, 0.1, 0.5], 3, 5, 0.15)[1:3] == (3, 0.0)
    assert ck.pick([1.0, 1.0, 0.01, 0.1, 0.12, 0.5], 3, 5, 0.15)[1:3] == (3, 0.0)
    # the clamp: a far above c
    assert ck.pick([1.0, 1.0, 0.9, 0.1, 0.1, 0.5], 3, 5, 0.15)[1:3] == (3, 0.5)


def test_checker_cmnd_definition():
    d = np.array([0.0, 2.0, 2.0, 0.0, 4.0])
    assert ck.cmnd(d).tolist() == [1.0, 1.0, 1.0, 0.0, 2.0]
    assert ck.cmnd(np.zeros(5)).tolist() == [1.0] * 5
    assert ck.cmnd(np.array([0.0, 0.0, 3.0])).tolist() == [1.0, 1.0, 2.0]       # a zero running sum gives 1, not 0 / 0


@pytest.mark.parametrize("hz", (82.4, 110.0, 220.5, 317.0, 440.0))
def test_checker_finds_five_harmonic_tones(hz):
    n = np.arange(8192)
    x = 0.2 * sum(np.sin(2 * np.pi * hz * h * n / ck.SR) / h for h in range(1, 6))
    f0, ap, dp, tau = ck.track(x)
    inner = interior(x.size, 367)
    assert len(inner) >= 20
    rel = np.abs(f0[inner] - hz) / hz
    print("%.1f Hz: largest relative error of the float64 checker on %d interior frames %.2e" % (hz, len(inner), rel.max()))
    assert (f0[inner] > 0).all() and rel.max() <= 1e-3


def test_frame_grid_is_the_front_end_s():
    from data_preprocessing.audio2mel import num_frames
    for n in (385, 512, 640, 16128, 16384, 33357):
        assert ck.frames_of(n) == num_frames(n) == _hip.lib().mcvc_audio_frames(n)
    assert ck.lags() == (45, 367) and ck.lags(35, 800) == (28, 630) and ck.lags(200, 250) == (89, 110)
    assert pitch.lag_range(60, 500) == (45, 367) and pitch.lag_range(35, 800) == (28, 630) and pitch.lag_range(200, 250) == (89, 110)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_bound():
    L = _hip.lib()
    for name in F0_SYMBOLS:
        assert name in _hip.EXPORTED_SYMBOLS and getattr(L, name).argtypes is not None
    assert L.mcvc_version() == 3
    assert L.mcvc_f0_max_lag() == 640 == pitch.MAX_LAG == ck.MAX_LAG
    assert L.mcvc_f0_launches(0) == 1 and L.mcvc_f0_launches(1) == 1


def test_track_refuses_before_it_touches_a_device():
    """Every refusal comes from the argument check: the device pointers are never followed, no device is needed."""
    L = _hip.lib()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16

    def run(wave=p, ns=4096, tiles=p, nt=1, lo=45, hi=367, thr=0.15, f0=p, ap=p, cm=p, total=15):
        return L.mcvc_f0_track(wave, ns, tiles, nt, lo, hi, thr, f0, ap, cm, total, None)

    for kw in (dict(wave=None), dict(tiles=None), dict(f0=None), dict(ap=None)):                             # null pointers
        assert run(**kw) == MCVC_ERR_INVALID, kw
    for kw in (dict(wave=p + 2), dict(f0=p + 1), dict(ap=p + 2), dict(cm=p + 3), dict(tiles=p + 8), dict(tiles=p + 4)):     # misaligned
        assert run(**kw) == MCVC_ERR_INVALID, kw
    for lo, hi in ((1, 367), (0, 10), (-5, 367), (45, 45), (46, 45), (45, 641), (45, 100000), (640, 640)):  # the lag rule
        assert run(lo=lo, hi=hi) == MCVC_ERR_INVALID, (lo, hi)
    for thr in (0.0, -0.15, 1.0000001, 2.0, float("nan"), float("inf"), -float("inf")):
        assert run(thr=thr) == MCVC_ERR_INVALID, thr
    assert run(nt=0) == MCVC_ERR_INVALID and run(nt=-1) == MCVC_ERR_INVALID
    assert run(total=0) == MCVC_ERR_INVALID and run(total=-3) == MCVC_ERR_INVALID
    assert run(ns=384) == MCVC_ERR_INVALID
    assert run(cm=None, thr=float("nan")) == MCVC_ERR_INVALID                                                 # (cmnd may be null; the rest is still checked)


def test_stats_refuses_before_it_touches_a_device():
    L = _hip.lib()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16

    def run(fx=p, nx=10, fy=p, ny=10, path=p, pairs=p, n=1, counts=p, sums=p):
        return L.mcvc_f0_stats(fx, nx, fy, ny, path, pairs, n, counts, sums, None)

    for kw in (dict(fx=None), dict(fy=None), dict(path=None), dict(pairs=None), dict(counts=None), dict(sums=None)):
        assert run(**kw) == MCVC_ERR_INVALID, kw
    for kw in (dict(fx=p + 2), dict(fy=p + 1), dict(path=p + 4), dict(pairs=p + 8), dict(counts=p + 2), dict(sums=p + 3)):
        assert run(**kw) == MCVC_ERR_INVALID, kw
    assert run(nx=0) == MCVC_ERR_INVALID and run(ny=0) == MCVC_ERR_INVALID and run(n=0) == MCVC_ERR_INVALID and run(n=-2) == MCVC_ERR_INVALID


# ---- parser and module ------------------------------------------------------------------------------------------------------------------
def test_evaluate_parser_f0_flags():
    p = EvaluateArgParser()
    d = p.parser.parse_args([])
    assert d.f0 is False and d.converted_audio_dir is None and d.f0_min == 60.0 and d.f0_max == 500.0 and d.f0_threshold == 0.15
    assert d.n_cep == 24 and d.converted_dir is None and d.target_speaker_id is None and d.target_wav_dir is None and d.source_speaker_id is None
    assert d.name == "debug" and d.preprocessed_data_dir == "vcc2018_training_preprocessed/"
    a = p.parse_args(["--target_speaker_id", "VCC2TF1"])                                                     # today's run parses as before
    assert a.f0 is False and a.target_speaker_id == "VCC2TF1" and a.n_cep == 24
    a = p.parse_args(["--target_wav_dir", "wavs", "--f0", "--f0_min", "70", "--f0_max", "400", "--f0_threshold", "0.2", "--converted_audio_dir", "aud"])
    assert a.f0 is True and (a.f0_min, a.f0_max, a.f0_threshold, a.converted_audio_dir) == (70.0, 400.0, 0.2, "aud")
    for bad in (["--target_speaker_id", "VCC2TF1", "--f0"],                                                  # --f0 needs audio references
                ["--target_wav_dir", "wavs", "--f0", "--f0_min", "500", "--f0_max", "60"],
                ["--target_wav_dir", "wavs", "--f0", "--f0_min", "20"],                                      # lag 1102 > 640
                ["--target_wav_dir", "wavs", "--f0", "--f0_max", "30000"],                                   # lag 2 is the shortest
                ["--target_wav_dir", "wavs", "--f0", "--f0_min", "60", "--f0_max", "60.1"],                  # no two lags
                ["--target_wav_dir", "wavs", "--f0", "--f0_threshold", "0"],
                ["--target_wav_dir", "wavs", "--f0", "--f0_threshold", "1.5"],
                ["--target_wav_dir", "wavs", "--f0", "--f0_threshold", "nan"]):
        with pytest.raises(SystemExit):
            EvaluateArgParser().parse_args(bad)


def test_lag_range_and_threshold_rules():
    for fmin, fmax in ((500, 60), (60, 60), (0, 500), (-1, 500), (34, 500), (60, 22050), (float("nan"), 500), (60, float("inf"))):
        with pytest.raises(ValueError):
            pitch.lag_range(fmin, fmax)
    assert pitch.lag_range(34.5, 11025) == (2, 639)
    for thr in (0, -1, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pitch.check_threshold(thr)
    assert pitch.check_threshold(1) == 1.0


def test_module_has_no_cpu_path_and_checks_its_input():
    x = [np.zeros(4096, dtype=np.float32)]
    with pytest.raises(ValueError):
        pitch.PitchTracker(fmin=20.0)                                                                         # the range is refused first
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            pitch.PitchTracker()
        with pytest.raises(RuntimeError, match="no CPU path"):
            metrics.f0_stats([np.zeros(3)], [np.zeros(3)], [np.zeros((3, 2), dtype=np.int32)])
        with pytest.raises(RuntimeError, match="no CPU path"):
            metrics.f0_distortion(x, x, [np.zeros((80, 16), dtype=np.float32)], [np.zeros((80, 16), dtype=np.float32)])
    else:
        tr = pitch.PitchTracker()
        assert tr.lags == (45, 367)
        with pytest.raises(RuntimeError, match="no CPU path"):
            pitch.PitchTracker(device="cpu")
        with pytest.raises(RuntimeError, match="no CPU path"):
            tr.track(torch.zeros(4096), [4096])
        with pytest.raises(ValueError, match="at least 385"):
            tr.bank([np.zeros(384, dtype=np.float32)])
        with pytest.raises(ValueError, match="finite"):
            tr.bank([np.full(4096, np.inf, dtype=np.float32)])
        with pytest.raises(ValueError, match="utterance 0"):
            metrics.f0_distortion(x, x, [np.zeros((80, 15), dtype=np.float32)], [np.zeros((80, 16), dtype=np.float32)])
        assert tr.bank([]) == []
