"""GPU: the silence detector (csrc/vad_kernels.hip via data_preprocessing.silence.SilenceDetector), the segmented log-mel launch
(``Audio2Mel.bank(trim_db=)``, ``bank_at_rates(trim_db=)``, ``bank_split``) and the ``--trim_silence`` / ``--split_silence`` command lines.

The truth is tests/silence_checker.py: float64 energies of the same float32 input.  The gates are derived there, not measured:

    |mse32 - mse64| <= 1.01 (2048 + 3) 2^-24 mse64   per frame, and for ref (any summation order, FMA or not)
    decisions are compared on inputs that have NO frame within band_db() = 10 log10((1 + g)^2 (1 + 2^-23)) ~ 1.1e-3 dB of the threshold;
    that is asserted on the float64 side first, so nothing is skipped silently.

Every case prints its largest error over its gate before it asserts; MCVC_VAD_ERROR_JSON=<path> records the per-case maxima (how
profiles/vad_error.json is made)."""
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
import silence_checker as ck  # noqa: E402
from data_preprocessing import preprocess_vcc2018, silence  # noqa: E402
from data_preprocessing.audio2mel import Audio2Mel, num_frames, read_wav  # noqa: E402
from data_preprocessing.resample import Resampler  # noqa: E402
from data_preprocessing.silence import SilenceDetector  # noqa: E402
from mask_cyclegan_vc import _hip  # noqa: E402
from mask_cyclegan_vc.train import load_speaker  # noqa: E402

WORST = {}


@pytest.fixture(scope="module")
def det():
    return SilenceDetector()


@pytest.fixture(scope="module")
def clips(golden_dir):
    """The two committed recordings as float32, and the int16 PCM of a long file made of both joined by 0.5 s of low noise."""
    pcm = []
    for name in ("real_VCC2SF3.wav", "real_VCC2TF1.wav"):
        rate, p = wavfile.read(os.path.join(golden_dir, "audio", name))
        assert rate == 22050 and p.dtype == np.int16
        pcm.append(p)
    room = np.random.RandomState(5).randint(-3, 4, size=11025).astype(np.int16)
    joined = np.concatenate([pcm[0], room, pcm[1]])
    to_float = lambda p: (p.astype(np.float64) / 32768.0).astype(np.float32)
    return {"a": to_float(pcm[0]), "b": to_float(pcm[1]), "pcm": pcm, "joined_pcm": joined, "joined": to_float(joined)}


def tile_frames():
    return _hip.lib().mcvc_vad_tile_frames()


def signal_of(n, seed, dc=0.01):
    """Seeded noise with loud and quiet stretches and a DC offset."""
    rs = np.random.RandomState(seed)
    env = np.where(((np.arange(n) + 3000) // 4000) % 2 == 1, 0.5, 1e-3)                # loud: samples 1000 .. 4999, 9000 .. 12999, ...
    return (env * rs.randn(n) + dc).astype(np.float32)


def lengths():
    TF = tile_frames()
    return [1, 511, 512, 513, 1024, 2047, 2048, 2049, 512 * TF - 1, 512 * TF, 512 * TF + 1, 1024 * TF + 513, 20001]


def record(case, worst):
    WORST[case] = max(WORST.get(case, 0.0), worst)
    path = os.environ.get("MCVC_VAD_ERROR_JSON")
    if path:
        with open(path, "w") as fh:
            json.dump(dict(worst_error_over_gate=WORST, gate="1.01 (2048 + 3) 2^-24 mse64 per frame and for ref, against the float64 checker",
                           note="largest over the cases of tests/test_hip_silence.py run so far"), fh, indent=1)


@pytest.fixture(scope="module")
def inputs():
    return [signal_of(n, 100 + n) for n in lengths()]


@pytest.fixture(scope="module")
def singles(det, inputs):
    """Every input through a launch of its own: computed once, shared, never changed."""
    out = []
    for x in inputs:
        (m,), ref = det.energies([x])
        out.append((m, ref[0]))
    return out


# ---- 1. energies against float64 -------------------------------------------------------------------------------------------------------
def test_energies_against_float64(inputs, singles):
    L = _hip.lib()
    assert L.mcvc_vad_launches() in (1, 2)
    worst = 0.0
    for x, (m, ref) in zip(inputs, singles):
        assert m.shape == (L.mcvc_vad_frames(x.size),) and ref == m.max()
        worst = max(worst, ck.check_energies("noise n=%d" % x.size, m, ref, x))
    record("lengths", worst)


# ---- 2. decisions ----------------------------------------------------------------------------------------------------------------------
def test_decisions_equal_the_checker(det, inputs, singles, clips):
    cases = [("noise n=%d" % x.size, x, 20.0, s) for x, s in zip(inputs, singles)]
    for name in ("a", "b"):
        (m,), ref = det.energies([clips[name]])
        worst = ck.check_energies("recording " + name, m, ref[0], clips[name])
        record("recordings", worst)
        cases += [("recording %s" % name, clips[name], top_db, (m, ref[0])) for top_db in (40.0, 60.0)]
    for name, x, top_db, _ in cases:
        ck.assert_decidable(name, x, top_db)                            # on the float64 side, for every input, before anything is compared
    for name, x, top_db, (m, ref) in cases:
        flags = det.nonsilent(m, ref, top_db)
        assert np.array_equal(flags, ck.nonsilent(ck.mse(x), top_db)), (name, top_db)
        assert silence.trim_bounds(flags, x.size) == ck.trim(x, top_db), (name, top_db)
        assert silence.split_intervals(flags, x.size) == ck.split(x, top_db), (name, top_db)
        assert np.abs(det.frame_db(m, ref) - ck.db(ck.mse(x))).max() <= 1e-2
    assert det.trim([clips["a"], clips["b"]], 40) == [(3072, 53248), (4096, 50176)]
    assert det.trim([clips["a"], clips["b"]], 60) == [(0, 54784), (1024, 51712)]
    ck.assert_decidable("joined recording", clips["joined"], 40.0)
    kept, dropped = det.split([clips["joined"], clips["a"]], 40, return_dropped=True)
    want = [ck.split_merged(clips["joined"], 40.0), ck.split_merged(clips["a"], 40.0)]
    assert kept == [w[0] for w in want] and dropped == [w[1] for w in want] and len(kept[0]) == 2 and len(kept[1]) == 1


# ---- 3. a bank equals its single calls, bit for bit ---------------------------------------------------------------------------------------
def test_bank_equals_single_launches(det, inputs, singles):
    n = len(inputs)
    for order in (list(range(n)), list(range(n))[::-1], [(7 * i + 3) % n for i in range(n)]):
        assert sorted(order) == list(range(n))
        mse, ref = det.energies([inputs[i] for i in order])
        assert ref.dtype == np.float32 and ref.shape == (n,)
        for k, i in enumerate(order):
            assert np.array_equal(mse[k], singles[i][0]) and ref[k] == singles[i][1], (i, inputs[i].size)
    # the same utterance at bank offsets 0 .. 3: the summation order does not follow the pointer's alignment
    for i in (3, 7, 12):
        for shift in (1, 2, 3):
            mse, ref = det.energies([np.full(shift, 0.7, dtype=np.float32), inputs[i]])
            assert np.array_equal(mse[1], singles[i][0]) and ref[1] == singles[i][1], (i, shift)
    # a device bank with lengths is the same call
    wave = torch.from_numpy(np.concatenate(inputs[:5])).cuda()
    mse, ref = det.energies(wave, lengths=[x.size for x in inputs[:5]])
    assert all(np.array_equal(mse[i], singles[i][0]) and ref[i] == singles[i][1] for i in range(5))


def test_quiet_utterance_between_loud_neighbours(det):
    """Zero padding, not the neighbour at full scale, fills the quiet utterance's edge frames: one leaked sample would raise them 80 dB."""
    rs = np.random.RandomState(9)
    loud = [np.sign(rs.randn(4000)).astype(np.float32) for _ in range(2)]
    for n in (3000, 512 * tile_frames() + 100):
        quiet = (1e-4 * rs.randn(n)).astype(np.float32)
        (alone,), ref_alone = det.energies([quiet])
        mse, ref = det.energies([loud[0], quiet, loud[1]])
        assert np.array_equal(mse[1], alone) and ref[1] == ref_alone[0]
        record("quiet between loud", ck.check_energies("quiet n=%d" % n, mse[1], ref[1], quiet))
        assert ref[0] == 1.0 and ref[2] == 1.0


# ---- 4. edge values ----------------------------------------------------------------------------------------------------------------------
def test_edge_values(det):
    n = 20001
    (m,), ref = det.energies([np.zeros(n, dtype=np.float32)])
    assert ref[0] == 0.0 and (m == 0.0).all() and det.nonsilent(m, ref[0], 40).all()
    assert det.trim([np.zeros(n, dtype=np.float32)], 40) == [(0, n)] and det.split([np.zeros(n, dtype=np.float32)], 40) == [[(0, n)]]
    faint = (3e-6 * np.random.RandomState(2).randn(n)).astype(np.float32)
    (m,), ref = det.energies([faint])
    assert 0.0 < ref[0] < 1e-10 and det.nonsilent(m, ref[0], 40).all() and det.trim([faint], 40) == [(0, n)]
    record("faint", ck.check_energies("faint", m, ref[0], faint))
    one = np.zeros(n, dtype=np.float32)
    one[5000] = 1.0
    (m,), ref = det.energies([one])
    assert np.flatnonzero(m).tolist() == [8, 9, 10, 11] and (m[8:12] == np.float32(1.0 / 2048)).all() and ref[0] == np.float32(1.0 / 2048)
    assert np.flatnonzero(det.nonsilent(m, ref[0], 40)).tolist() == [8, 9, 10, 11] and det.trim([one], 40) == [(4096, 6144)]


# ---- 5. segmented log-mel ------------------------------------------------------------------------------------------------------------------
def test_trimmed_bank_equals_host_sliced_bank(clips):
    fft = Audio2Mel()
    ws = [clips["a"], clips["b"], clips["a"][:30000]]
    for w in ws:
        ck.assert_decidable("recording", w, 40.0)
    bounds = [ck.trim(w, 40.0) for w in ws]
    got, got_bounds = fft.bank(ws, trim_db=40, return_bounds=True)
    want = fft.bank([w[s:e] for w, (s, e) in zip(ws, bounds)])
    assert got_bounds == bounds and len(got) == 3
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and np.array_equal(g, w)
    plain = fft.bank(ws, trim_db=40)
    assert all(np.array_equal(g, w) for g, w in zip(plain, want))
    assert [g.shape[1] for g in got[:2]] == [(53248 - 3072) // 256, (50176 - 4096) // 256]


def test_trimmed_bank_at_rates(clips):
    fft, rs = Audio2Mel(), Resampler()
    x = clips["a"]
    x16 = signal.resample_poly(x.astype(np.float64), 320, 441).astype(np.float32)
    (back16,) = rs.bank([x16], 16000, 22050, to_host=True)
    for w in (back16, x):
        ck.assert_decidable("recording", w, 40.0)
    bounds = [ck.trim(back16, 40.0), ck.trim(x, 40.0)]
    got, got_bounds = fft.bank_at_rates([x16, x], [16000, 22050], trim_db=40, return_bounds=True)
    want = fft.bank([back16[bounds[0][0]:bounds[0][1]], x[bounds[1][0]:bounds[1][1]]])
    assert got_bounds == bounds
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_bank_split_on_a_joined_file(clips):
    fft = Audio2Mel()
    j = clips["joined"]
    ck.assert_decidable("joined recording", j, 40.0)
    kept, dropped = ck.split_merged(j, 40.0)
    assert len(kept) == 2
    mels, intervals, index, stats = fft.bank_split([j, clips["b"]], 40, return_segments=True)
    own, own_dropped = ck.split_merged(clips["b"], 40.0)
    assert intervals == kept + own and index == [0, 0] + [1] * len(own) and stats == {"dropped": [dropped, own_dropped], "samples": [j.size, clips["b"].size]}
    want = fft.bank([j[s:e] for s, e in kept] + [clips["b"][s:e] for s, e in own])
    assert len(mels) == len(want) and all(np.array_equal(g, w) for g, w in zip(mels, want))
    assert all(np.array_equal(g, w) for g, w in zip(fft.bank_split([j, clips["b"]], 40), want))


def test_refusals(det, clips):
    fft = Audio2Mel()
    x = clips["a"]
    with pytest.raises(RuntimeError, match="no CPU path"):
        det.energies(torch.from_numpy(x), lengths=[x.size])
    with pytest.raises(RuntimeError, match="no CPU path"):
        det.launch(torch.from_numpy(x), [x.size])
    for bad in (0, -40, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="top_db"):
            det.trim([x], bad)
        with pytest.raises(ValueError, match="top_db"):
            det.split([x], bad)
        with pytest.raises(ValueError, match="top_db"):
            fft.bank([x], trim_db=bad)
        with pytest.raises(ValueError, match="top_db"):
            fft.bank_split([x], bad)
    with pytest.raises(ValueError, match="none empty"):
        det.energies(torch.from_numpy(x).cuda(), lengths=[x.size, 0])
    wave = torch.from_numpy(x).cuda()
    with pytest.raises(ValueError, match="at least 385 samples"):
        fft._launch_segments(wave, [0, 1000], [5000, 384])
    with pytest.raises(ValueError, match="outside the bank"):
        fft._launch_segments(wave, [x.size - 1000], [1001])
    out, fo = fft._launch_segments(wave, [1000, 0], [5000, x.size])        # overlapping, reordered: fine
    assert np.array_equal(out.cpu().numpy()[:, fo[1]:fo[2]], fft.bank([x])[0])


# ---- 6. the command lines ------------------------------------------------------------------------------------------------------------------
def _wav_folder(root, clips, joined=False):
    os.makedirs(os.path.join(root, "SPK"))
    if joined:
        wavfile.write(os.path.join(root, "SPK", "long.wav"), 22050, clips["joined_pcm"])
    else:
        for name, p in zip(("a.wav", "b.wav"), clips["pcm"]):
            wavfile.write(os.path.join(root, "SPK", name), 22050, p)


def test_preprocess_cli_trim_and_split(tmp_path, clips, capsys):
    _wav_folder(str(tmp_path / "wavs"), clips)
    common = ["--preprocessed_data_directory", str(tmp_path / "out"), "--speaker_ids", "SPK"]
    for extra in ([], ["--gpu_resample"]):
        preprocess_vcc2018.main(["--data_directory", str(tmp_path / "wavs"), "--trim_silence", "40"] + common + extra)
        mels, mean, std = load_speaker(str(tmp_path / "out"), "SPK")
        frames = [num_frames(e - s) for s, e in (ck.trim(clips[k], 40.0) for k in ("a", "b"))]
        assert [m.shape for m in mels] == [(80, f) for f in frames] and frames == [196, 180]
        want, wmean, wstd = preprocess_vcc2018.normalize_mels(Audio2Mel().bank([clips["a"][3072:53248], clips["b"][4096:50176]]))
        assert np.array_equal(mean, wmean) and np.array_equal(std, wstd) and all(np.array_equal(m, w) for m, w in zip(mels, want))
    _wav_folder(str(tmp_path / "long"), clips, joined=True)
    capsys.readouterr()
    for extra in ([], ["--gpu_resample"]):
        preprocess_vcc2018.main(["--data_directory", str(tmp_path / "long"), "--split_silence", "40", "--min_silence_ms", "300"] + common + extra)
        out = capsys.readouterr().out
        kept, dropped = ck.split_merged(clips["joined"], 40.0)
        share = 100.0 * sum(e - s for s, e in kept) / clips["joined"].size
        assert "1 files -> 2 utterances, %d intervals dropped" % dropped in out and "%.1f %% of the samples kept" % share in out
        mels, _, _ = load_speaker(str(tmp_path / "out"), "SPK")
        assert [m.shape for m in mels] == [(80, num_frames(e - s)) for s, e in kept] and len(mels) == 2


def test_inference_cli_trim_silence(tmp_path, clips):
    from mask_cyclegan_vc import test as test_cli
    _wav_folder(str(tmp_path / "clips"), clips)
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
    test_cli.main(["--name", "trim", "--save_dir", str(tmp_path / "res"), "--preprocessed_data_dir", data, "--speaker_A_id", "SPKA", "--speaker_B_id", "SPKB",
                   "--ckpt_dir", str(ck_dir), "--load_epoch", "1", "--model_name", "generator_A2B", "--wav_dir", str(tmp_path / "clips"),
                   "--trim_silence", "40"])
    d = str(tmp_path / "res" / "trim" / "converted_mel")
    got = [np.load(os.path.join(d, "%d-converted_SPKA_to_SPKB.npy" % i)).shape for i in (0, 1)]
    assert got == [(80, 196), (80, 180)]


def test_evaluate_cli_trim_silence(tmp_path, clips):
    from mask_cyclegan_vc import evaluate
    fft = Audio2Mel()
    waves = [clips["a"], clips["b"]]
    mels = fft.bank(waves)
    run_dir = tmp_path / "run" / "exp"
    for sub in ("converted_mel", "converted_audio"):
        os.makedirs(str(run_dir / sub))
    os.makedirs(str(tmp_path / "tgt"))
    for i in range(2):
        np.save(str(run_dir / "converted_mel" / ("%d-converted_SRC_to_TGT.npy" % i)), mels[i])
        wavfile.write(str(run_dir / "converted_audio" / ("%d-converted_SRC_to_TGT.wav" % i)), 22050, waves[i])
        wavfile.write(str(tmp_path / "tgt" / ("%02d.wav" % i)), 22050, clips["pcm"][i])
    base = ["--save_dir", str(tmp_path / "run"), "--name", "exp", "--target_wav_dir", str(tmp_path / "tgt")]
    plain = evaluate.main(base + ["--f0"])
    assert "trim_silence_db" not in plain and [u["frames_target"] for u in plain["utterances"]] == [224, 225]
    rep = evaluate.main(base + ["--f0", "--trim_silence", "40"])
    disk = json.load(open(str(run_dir / "metrics.json")))
    assert disk == json.loads(json.dumps(rep)) and disk["trim_silence_db"] == 40.0
    assert [u["frames_target"] for u in disk["utterances"]] == [196, 180] and [u["frames_converted"] for u in disk["utterances"]] == [224, 225]
    assert "f0" in disk and all("vuv_error" in u for u in disk["utterances"])
