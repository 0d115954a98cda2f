"""GPU checks of the pitch tracker (csrc/f0_kernels.hip through mask_cyclegan_vc/pitch.py, metrics.f0_stats / f0_distortion and the evaluate
CLI's --f0) against the float64 restatement tests/f0_checker.py.

Shapes: the smallest at which a tracker working in sub-tiles of 8 frames inside plan tiles of 64 can go wrong -- 385, 512 and 640 samples
(one and two frames, the window almost wholly in the zero padding), 256 T samples for T = 63, 64, 65 (one short of a plan tile, a full one,
one over) and 256 * 130 + 77 (three tiles, a ragged tail) -- at the lag ranges of (60, 500) Hz = 45 .. 367, (35, 800) Hz = 28 .. 630 (near the
limit of 640) and (200, 250) Hz = 89 .. 110 (narrower than a wavefront).

The d' gate |err| <= (2 W + tau + 16) 2^-24 d'64 is derived, not measured: d sums W positive terms that carry two roundings each (the
difference, the fused square-and-add) in some order, the running sum adds at most tau positive terms, one multiply, one divide, and a margin
of 12.  The decisions are then checked WITHOUT tolerance: the checker's pick rule runs on the d' the kernel returned."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import f0_checker as ck  # noqa: E402
from data_preprocessing.audio2mel import Audio2Mel, read_wav  # noqa: E402
from mask_cyclegan_vc import _hip, evaluate, metrics, pitch  # noqa: E402

U24 = 2.0 ** -24
LENGTHS = (385, 512, 640, 256 * 63, 256 * 64, 256 * 65, 256 * 130 + 77)
RANGES = ((60.0, 500.0), (35.0, 800.0), (200.0, 250.0))
TONES = {RANGES[0]: (97.0, 140.0, 233.0, 110.0, 180.0, 310.0, 150.0), RANGES[1]: (52.0, 640.0, 75.0, 44.0, 400.0, 90.0, 61.0),
         RANGES[2]: (225.0, 222.0, 228.0, 224.0, 226.0, 223.0, 227.0)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio")


def tone(n, hz, seed, vibrato=0.03, cycles_per_s=5.0, noise_db=-30.0):
    """Five harmonics (1 / h) of a tone with `vibrato` relative frequency modulation, plus white noise `noise_db` below its RMS; float32."""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / ck.SR
    phase = 2 * np.pi * np.cumsum(hz * (1.0 + vibrato * np.sin(2 * np.pi * cycles_per_s * t))) / ck.SR
    x = 0.2 * sum(np.sin(h * phase) / h for h in range(1, 6))
    x = x + rs.randn(n) * np.sqrt(np.mean(x * x)) * 10.0 ** (noise_db / 20.0)
    return x.astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def run(tracker, waves):
    """One launch with cmnd -> per utterance (f0 [T], aperiodicity [T], d' [tau_max + 1, T]) numpy float32."""
    f0, ap, fo, cm = tracker.track(torch.from_numpy(np.concatenate(waves)).cuda(), [w.size for w in waves], return_cmnd=True)
    f0, ap, cm = f0.cpu().numpy(), ap.cpu().numpy(), cm.cpu().numpy()
    return [(f0[fo[i]:fo[i + 1]], ap[fo[i]:fo[i + 1]], cm[:, fo[i]:fo[i + 1]]) for i in range(len(waves))]


@pytest.fixture(scope="module")
def waves():
    return {r: [tone(n, hz, 100 * k + i) for i, (n, hz) in enumerate(zip(LENGTHS, TONES[r]))] for k, r in enumerate(RANGES)}


@pytest.fixture(scope="module")
def trackers():
    return {r: pitch.PitchTracker(fmin=r[0], fmax=r[1]) for r in RANGES}


@pytest.fixture(scope="module")
def single(waves, trackers):
    """Every utterance as a call of its own."""
    return {r: [run(trackers[r], [w])[0] for w in waves[r]] for r in RANGES}


@pytest.fixture(scope="module")
def want(waves, trackers):
    """float64 d' on the same float32 samples, computed once: range -> [d' [tau_max + 1, T]]."""
    out = {}
    for r in RANGES:
        lo, hi = trackers[r].lags
        out[r] = [ck.track(w, lo, hi, 0.15)[2] for w in waves[r]]
    return out


def test_lag_ranges(trackers):
    assert [trackers[r].lags for r in RANGES] == [(45, 367), (28, 630), (89, 110)]
    assert _hip.lib().mcvc_f0_launches(1) == 1


@pytest.mark.parametrize("r", RANGES)
def test_cmnd_element_by_element(single, want, trackers, r):
    lo, hi = trackers[r].lags
    tau = np.arange(hi + 1, dtype=np.float64)[:, None]
    worst = 0.0
    for n, (f0, ap, cm), dp64 in zip(LENGTHS, single[r], want[r]):
        assert cm.shape == dp64.shape == (hi + 1, ck.frames_of(n)) and cm.dtype == np.float32
        gate = (2 * ck.W + tau + 16) * U24 * dp64
        err = np.abs(cm.astype(np.float64) - dp64)
        exact = (dp64 == 0.0) | (tau == 0)                                    # 0 and 1 by definition: no tolerance there
        assert (cm[0] == 1.0).all() and (err[exact] == 0.0).all()
        ratio = float((err[~exact] / gate[~exact]).max())
        worst = max(worst, ratio)
        assert (err <= gate).all(), (n, ratio)
    print("range %g .. %g Hz (lags %d .. %d): largest d' error / gate %.4f" % (r[0], r[1], lo, hi, worst))


@pytest.mark.parametrize("r", RANGES)
def test_decisions_exactly_on_the_returned_cmnd(single, trackers, r):
    """The checker's pick on the kernel's own d': voiced flag and lag identical, aperiodicity bit-equal, f0 within 16 x 2^-24.  Every frame."""
    lo, hi = trackers[r].lags
    frames = voiced_frames = 0
    worst = 0.0
    for n, (f0, ap, cm) in zip(LENGTHS, single[r]):
        for t in range(f0.size):
            voiced, tau, off, f64, a64 = ck.pick(cm[:, t].astype(np.float64), lo, hi, float(np.float32(0.15)))
            frames += 1
            assert (f0[t] > 0) == voiced, (n, t)
            assert bits(ap[t:t + 1])[0] == bits(np.array([a64]))[0], (n, t, ap[t], a64)
            if not voiced:
                assert f0[t] == 0.0
                continue
            voiced_frames += 1
            rel = abs(float(f0[t]) - f64) / f64
            worst = max(worst, rel)
            assert rel <= 16 * U24, (n, t, f0[t], f64)
            if abs(off) < 0.49:                                               # (the lag read back from f0; at the clamp it is ambiguous)
                assert int(round(ck.SR / float(f0[t]))) == tau, (n, t)
            assert ap[t] == cm[tau, t]
    print("range %g .. %g Hz: %d frames, %d voiced; largest f0 error / (16 x 2^-24) %.4f" % (r[0], r[1], frames, voiced_frames, worst / (16 * U24)))
    assert voiced_frames >= frames // 2                                       # the tones are found: not an all-unvoiced pass


@pytest.mark.parametrize("name,lo_voiced,hi_voiced", [("real_VCC2SF3.wav", 40, 120), ("real_VCC2TF1.wav", 40, 120)])
def test_real_speech_against_the_float64_run(name, lo_voiced, hi_voiced):
    """The whole recording at (60, 500) Hz against the pure float64 run.  A frame is DECISIVE if every pair the float64 pick compared differs
    by at least 6e-4 max(lhs, rhs) -- 4 x the derived d' bound at tau_max = 367; there the voiced flag and the lag must equal the checker's and
    f0 lies within 1e-4.  At most 2 % of the frames may be indecisive."""
    x = read_wav(os.path.join(GOLDEN, name))
    tr = pitch.PitchTracker()
    lo, hi = tr.lags
    f0, ap, cm = run(tr, [x])[0]
    f64, a64, dp64, tau64 = ck.track(x, lo, hi, 0.15)
    T = f0.size
    assert T == f64.size
    gate = (2 * ck.W + np.arange(hi + 1)[:, None] + 16) * U24 * dp64
    err = np.abs(cm.astype(np.float64) - dp64)
    nz = dp64 > 0
    print("%s: %d frames; largest d' error / gate %.4f" % (name, T, float((err[nz] / gate[nz]).max())))
    assert (err <= gate).all()
    decisive = 0
    worst = 0.0
    for t in range(T):
        pairs = ck.comparisons(dp64[:, t], lo, hi, 0.15)
        if not all(abs(a - b) >= 6e-4 * max(a, b) for a, b in pairs):
            continue
        decisive += 1
        assert (f0[t] > 0) == (tau64[t] > 0), t
        if tau64[t] > 0:
            rel = abs(float(f0[t]) - f64[t]) / f64[t]
            worst = max(worst, rel)
            assert rel <= 1e-4 and abs(ck.SR / float(f0[t]) - tau64[t]) <= 0.5 + 1e-3, (t, f0[t], f64[t])
    voiced = int((f0 > 0).sum())
    print("%s: %d of %d frames indecisive; %d voiced (float64: %d); largest f0 relative error on decisive frames %.2e"
          % (name, T - decisive, T, voiced, int((tau64 > 0).sum()), worst))
    assert T - decisive <= 0.02 * T
    assert lo_voiced <= voiced <= hi_voiced


def raw_run(tracker, ws, fill, want_cmnd):
    """The C ABI with buffers of this test's own, outputs pre-filled with ``fill`` (bytes)."""
    import ctypes
    L = _hip.lib()
    offs = np.zeros(len(ws) + 1, dtype=np.int32)
    np.cumsum([w.size for w in ws], out=offs[1:])
    fo = np.zeros(len(ws) + 1, dtype=np.int32)
    nt = ctypes.c_int(0)
    assert L.mcvc_audio_plan(offs.ctypes.data, len(ws), fo.ctypes.data, None, 0, ctypes.byref(nt)) == 0
    tiles = np.zeros((nt.value, 4), dtype=np.int32)
    assert L.mcvc_audio_plan(offs.ctypes.data, len(ws), fo.ctypes.data, tiles.ctypes.data, nt.value, ctypes.byref(nt)) == 0
    total = int(fo[-1])
    lo, hi = tracker.lags
    wave = torch.from_numpy(np.concatenate(ws)).cuda()
    td = torch.from_numpy(tiles).cuda()
    f0 = torch.full((total * 4,), fill, dtype=torch.uint8, device="cuda")
    ap = torch.full((total * 4,), fill, dtype=torch.uint8, device="cuda")
    cm = torch.full(((hi + 1) * total * 4,), fill, dtype=torch.uint8, device="cuda") if want_cmnd else None
    rc = L.mcvc_f0_track(_hip.ptr(wave), int(offs[-1]), _hip.ptr(td), nt.value, lo, hi, tracker.threshold, _hip.ptr(f0), _hip.ptr(ap), _hip.ptr(cm),
                         total, _hip.stream())
    assert rc == 0
    torch.cuda.synchronize()
    f0, ap = f0.view(torch.float32).cpu().numpy(), ap.view(torch.float32).cpu().numpy()
    cm = cm.view(torch.float32).view(hi + 1, total).cpu().numpy() if want_cmnd else None
    return [(f0[fo[i]:fo[i + 1]], ap[fo[i]:fo[i + 1]], None if cm is None else cm[:, fo[i]:fo[i + 1]]) for i in range(len(ws))]


@pytest.mark.parametrize("r", RANGES)
def test_ragged_bank_equals_its_single_calls(waves, single, trackers, r):
    """Shuffled order: a window that leaks into the neighbouring utterance of the bank would change an edge frame."""
    order = np.random.RandomState(5).permutation(len(LENGTHS))
    ws = [waves[r][i] for i in order]
    results = [("bank", run(trackers[r], ws))]
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        results.append(("side stream", run(trackers[r], ws)))
    torch.cuda.current_stream().wait_stream(st)
    for fill in (0xFF, 0x00):
        results.append(("raw %#x" % fill, raw_run(trackers[r], ws, fill, True)))
        results.append(("raw %#x no cmnd" % fill, raw_run(trackers[r], ws, fill, False)))
    for what, res in results:
        for k, i in enumerate(order):
            f0, ap, cm = res[k]
            assert np.array_equal(bits(f0), bits(single[r][i][0])) and np.array_equal(bits(ap), bits(single[r][i][1])), (what, LENGTHS[i])
            if cm is not None:
                assert np.array_equal(bits(cm), bits(single[r][i][2])), (what, LENGTHS[i])
    host = trackers[r].bank(ws)                                               # the numpy interface: the same launch
    for k, i in enumerate(order):
        assert np.array_equal(bits(host[k][0]), bits(single[r][i][0])) and np.array_equal(bits(host[k][1]), bits(single[r][i][1]))


def test_silence_and_dc_beside_a_tone(waves, single, trackers):
    r = RANGES[0]
    lo, hi = trackers[r].lags
    n = 4096
    t_tone = waves[r][4]
    res = run(trackers[r], [np.zeros(n, dtype=np.float32), t_tone, np.full(n, 0.37, dtype=np.float32)])
    (f0z, apz, cmz), (f0t, apt, cmt), (f0c, apc, cmc) = res
    assert (f0z == 0).all() and (apz == 1.0).all() and (cmz == 1.0).all()
    # a constant meets the zero padding in the edge frames (d' = 2 tau / (tau + 1) there: unvoiced too); where the window is inside, d is 0
    inner = [t for t in range(f0c.size) if ck.HOP * t + ck.HOP // 2 - (ck.W + hi) // 2 >= 0 and ck.HOP * t + ck.HOP // 2 - (ck.W + hi) // 2 + ck.W + hi <= n]
    assert len(inner) >= 8 and (f0c == 0).all() and (apc[inner] == 1.0).all() and (cmc[:, inner] == 1.0).all()
    assert np.array_equal(bits(f0t), bits(single[r][4][0])) and np.array_equal(bits(apt), bits(single[r][4][1])) and np.array_equal(bits(cmt), bits(single[r][4][2]))


# ---- F0 statistics along paths --------------------------------------------------------------------------------------------------------------
def diagonal(n):
    return np.stack([np.arange(n, dtype=np.int32)] * 2, axis=1)


def test_f0_stats_hand_built_octave():
    rs = np.random.RandomState(21)
    fxs, fys, paths, counts = [], [], [], []
    for n in (1, 63, 64, 65, 200):
        fy = rs.uniform(80.0, 300.0, n).astype(np.float32)
        fx = (2.0 * fy).astype(np.float32)                                    # exact: one octave up
        kind = rs.randint(0, 4, n)                                            # 0 both voiced, 1 x only, 2 y only, 3 neither
        kind[0] = 0
        fx[(kind == 2) | (kind == 3)] = 0.0
        fy[(kind == 1) | (kind == 3)] = 0.0
        fxs.append(fx); fys.append(fy); paths.append(diagonal(n))
        counts.append([int((kind == c).sum()) for c in range(4)])
    fxs.append(np.array([0.0, 100.0, 0.0], dtype=np.float32)); fys.append(np.array([120.0, 0.0, 0.0], dtype=np.float32)); paths.append(diagonal(3))
    counts.append([0, 1, 1, 1])                                               # a pair without a both-voiced row
    res = metrics.f0_stats(fxs, fys, [torch.from_numpy(p).cuda() for p in paths])
    assert res["counts"].tolist() == counts and res["length"].tolist() == [1, 63, 64, 65, 200, 3]
    assert res["voiced_pairs"].tolist() == [c[0] for c in counts]
    assert (res["bias_cents"][:5] == 1200.0).all() and (res["rmse_cents"][:5] == 1200.0).all()
    assert res["vuv_error"].tolist() == [(c[1] + c[2]) / float(sum(c)) for c in counts]
    assert np.isnan(res["bias_cents"][5]) and np.isnan(res["rmse_cents"][5]) and res["voiced_pairs"][5] == 0
    for k in range(6):                                                        # a batch equals its single calls
        one = metrics.f0_stats([fxs[k]], [fys[k]], [paths[k]])
        assert one["counts"][0].tolist() == counts[k]
        assert np.array_equal(one["bias_cents"], res["bias_cents"][k:k + 1], equal_nan=True) and np.array_equal(one["rmse_cents"], res["rmse_cents"][k:k + 1], equal_nan=True)


def test_f0_stats_random_tracks_against_float64():
    rs = np.random.RandomState(22)
    fxs, fys, paths = [], [], []
    for Tx, Ty in ((70, 83), (130, 120), (64, 65), (1, 5)):
        fxs.append(rs.uniform(80.0, 400.0, Tx).astype(np.float32))
        fys.append((rs.uniform(80.0, 400.0, Ty)).astype(np.float32))
        i = j = 0
        rows = [(0, 0)]
        while (i, j) != (Tx - 1, Ty - 1):                                     # a random monotone walk
            step = rs.randint(0, 3)
            if i < Tx - 1 and j < Ty - 1 and step == 0:
                i, j = i + 1, j + 1
            elif i < Tx - 1 and (step == 1 or j == Ty - 1):
                i += 1
            elif j < Ty - 1:
                j += 1
            rows.append((i, j))
        paths.append(np.array(rows, dtype=np.int32))
    fxs.append(rs.uniform(80.0, 400.0, 200).astype(np.float32))               # near unison: ratios close to 1, where log2 is small
    fys.append((fxs[-1] * (1.0 + 0.01 * rs.randn(200))).astype(np.float32))
    paths.append(diagonal(200))
    res = metrics.f0_stats(fxs, fys, paths)
    for k, (fx, fy, p) in enumerate(zip(fxs, fys, paths)):
        c = 1200.0 * np.log2(fx[p[:, 0]].astype(np.float64) / fy[p[:, 1]].astype(np.float64))
        rmse64, bias64, n = float(np.sqrt(np.mean(c * c))), float(np.mean(c)), len(p)
        gate = 1e-3 + (n + 32) * 2.0 ** -23 * rmse64
        print("pair %d: %d rows, rmse %.6f cents (float64 %.6f), bias %.6f (float64 %.6f), errors %.2e / %.2e, gate %.2e"
              % (k, n, res["rmse_cents"][k], rmse64, res["bias_cents"][k], bias64, abs(res["rmse_cents"][k] - rmse64), abs(res["bias_cents"][k] - bias64), gate))
        assert res["voiced_pairs"][k] == n and res["length"][k] == n and res["vuv_error"][k] == 0.0
        assert abs(res["rmse_cents"][k] - rmse64) <= gate and abs(res["bias_cents"][k] - bias64) <= gate
        one = metrics.f0_stats([fx], [fy], [p])
        assert one["rmse_cents"][0] == res["rmse_cents"][k] and one["bias_cents"][0] == res["bias_cents"][k]


# ---- the CLI, end to end --------------------------------------------------------------------------------------------------------------------
def sweep(n, hz, seed):
    """A vibrato tone whose spectral envelope moves with the position in the utterance, so that the DTW over mel cepstra has something to
    align: position u in [0, 1], f(u) = hz (1 + 0.03 sin(4 pi u)), harmonic h weighted by a bump centred on 1.5 + 5 u."""
    rs = np.random.RandomState(seed)
    u = np.arange(n) / float(n)
    phase = 2 * np.pi * np.cumsum(hz * (1.0 + 0.03 * np.sin(4 * np.pi * u))) / ck.SR
    x = 0.2 * sum(np.exp(-0.5 * ((h - (1.5 + 5.0 * u)) / 1.2) ** 2) * np.sin(h * phase) for h in range(1, 9))
    return (x + 1e-3 * rs.randn(n)).astype(np.float32)


def test_evaluate_cli_with_f0(tmp_path, capsys):
    from scipy.io import wavfile
    shift = 2.0 ** (300.0 / 1200.0)
    conv = [sweep(256 * T, hz, 40 + k) for k, (T, hz) in enumerate(((70, 120.0), (130, 180.0), (64, 240.0)))]
    tgt = [sweep(256 * T, hz * shift, 50 + k) for k, (T, hz) in enumerate(((83, 120.0), (120, 180.0), (65, 240.0)))]   # stretched, +300 cents
    fft = Audio2Mel()
    conv_mels, tgt_mels = fft.bank(conv), fft.bank(tgt)
    run_dir = tmp_path / "run" / "exp"
    for sub in ("converted_mel", "converted_audio"):
        os.makedirs(str(run_dir / sub))
    os.makedirs(str(tmp_path / "tgt"))
    for i in range(3):
        np.save(str(run_dir / "converted_mel" / ("%d-converted_SRC_to_TGT.npy" % i)), conv_mels[i])
        wavfile.write(str(run_dir / "converted_audio" / ("%d-converted_SRC_to_TGT.wav" % i)), ck.SR, conv[i])
        wavfile.write(str(run_dir / "converted_audio" / ("%d-original_SRC.wav" % i)), ck.SR, tgt[i])          # test.py writes these too: not read
        wavfile.write(str(tmp_path / "tgt" / ("%02d.wav" % i)), ck.SR, tgt[i])
    base = ["--save_dir", str(tmp_path / "run"), "--name", "exp", "--target_wav_dir", str(tmp_path / "tgt")]
    plain = evaluate.main(base)
    assert "F0" not in capsys.readouterr().out
    assert "f0" not in plain and all(not any(k.startswith("f0") or k in ("vuv_error", "voiced_pairs") for k in u) for u in plain["utterances"])
    rep = evaluate.main(base + ["--f0"])
    out = capsys.readouterr().out
    assert "MCD over 3 utterances" in out and "F0 RMSE" in out
    disk = json.load(open(str(run_dir / "metrics.json")))
    assert disk == json.loads(json.dumps(rep))
    assert [u["mcd"] for u in disk["utterances"]] == [u["mcd"] for u in plain["utterances"]] and disk["mean"] == plain["mean"]
    want = metrics.f0_distortion(conv, tgt, conv_mels, tgt_mels, 24)
    for k, u in enumerate(disk["utterances"]):
        print("utterance %d: F0 RMSE %.2f cents, bias %.2f cents, V/UV error %.4f over %d voiced of %d path rows"
              % (k, u["f0_rmse_cents"], u["f0_bias_cents"], u["vuv_error"], u["voiced_pairs"], u["length"]))
        assert u["f0_rmse_cents"] == float(want["rmse_cents"][k]) and u["f0_bias_cents"] == float(want["bias_cents"][k])
        assert u["vuv_error"] == float(want["vuv_error"][k]) and u["voiced_pairs"] == int(want["voiced_pairs"][k]) and u["length"] == int(want["length"][k])
        assert abs(u["f0_bias_cents"] + 300.0) <= 10.0
    f = disk["f0"]
    assert f["n_utterances_voiced"] == 3 and (f["tau_min"], f["tau_max"], f["threshold"]) == (45, 367, 0.15) and "unit" in f
    assert f["bias_cents"]["mean"] == float(want["bias_cents"].mean()) and f["rmse_cents"]["median"] == float(np.median(want["rmse_cents"]))
    assert abs(1200.0 * np.log2(f["median_f0_converted_hz"] / f["median_f0_target_hz"]) + 300.0) <= 60.0
    # a wav whose frame count differs from its mel's
    wavfile.write(str(run_dir / "converted_audio" / "1-converted_SRC_to_TGT.wav"), ck.SR, conv[1][:256 * 100])
    with pytest.raises(ValueError, match="utterance 1 .converted."):
        evaluate.main(base + ["--f0"])
    # a converted index without a wav
    os.remove(str(run_dir / "converted_audio" / "1-converted_SRC_to_TGT.wav"))
    with pytest.raises(ValueError, match="converted utterance 1 has no converted audio"):
        evaluate.main(base + ["--f0"])
