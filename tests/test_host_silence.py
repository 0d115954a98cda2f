"""CPU-only checks of the silence detector's host side (data_preprocessing/silence.py, the mcvc_vad_* / mcvc_audio_plan_segments C ABI, the
new command-line flags) and of the float64 checker itself (tests/silence_checker.py).  No kernel is launched here."""
import argparse
import ctypes
import os

import numpy as np
import pytest

import silence_checker as ck
from args.cycleGAN_test_arg_parser import CycleGANTestArgParser
from args.evaluate_arg_parser import EvaluateArgParser
from data_preprocessing import preprocess_vcc2018, silence
from data_preprocessing.audio2mel import read_wav
from mask_cyclegan_vc import _hip

MCVC_ERR_INVALID, MCVC_ERR_WORKSPACE = 1001, 1002
SYMBOLS = ("mcvc_vad_frame_length", "mcvc_vad_hop", "mcvc_vad_tile_frames", "mcvc_vad_launches", "mcvc_vad_frames", "mcvc_vad_plan", "mcvc_vad_energy",
           "mcvc_audio_plan_segments")
LENGTHS = (1, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 20001)
# trim bounds of the committed recordings, computed in float64 on the CPU when the feature was specified
GOLDEN_TRIM = {40: {"real_VCC2SF3": (3072, 53248), "real_VCC2TF1": (4096, 50176)}, 60: {"real_VCC2SF3": (0, 54784), "real_VCC2TF1": (1024, 51712)}}


def signal_of(n, seed):
    """Seeded noise with loud and quiet stretches and a DC offset."""
    rs = np.random.RandomState(seed)
    env = np.where(((np.arange(n) + 3000) // 4000) % 2 == 1, 0.5, 1e-3)                # loud: samples 1000 .. 4999, 9000 .. 12999, ...
    return (env * rs.randn(n) + 0.01).astype(np.float32)


def explicit_mse(x32):
    """The definition with every frame materialised: zero-pad 1024 each side, cut 2048-sample frames at hop 512, mean of squares."""
    x = np.asarray(x32, dtype=np.float32).astype(np.float64)
    L = x.size
    T = 1 + L // 512
    padded = np.zeros(512 * (T - 1) + 2048 + 1024)
    padded[1024:1024 + L] = x
    return np.array([np.mean(padded[512 * t:512 * t + 2048] ** 2) for t in range(T)])


@pytest.mark.parametrize("n", LENGTHS)
def test_checker_equals_explicit_frames(n):
    L = _hip.lib()
    x = signal_of(n, n)
    want = explicit_mse(x)
    got = ck.mse(x)
    assert got.shape == want.shape == (ck.frames(n),) == (silence.num_frames(n),) == (L.mcvc_vad_frames(n),)
    err = float(np.abs(got - want).max())
    print("n = %d: |cumsum - explicit| <= %.2e of max %.2e" % (n, err, want.max()))
    assert err <= 1e-12 * want.max()                                   # (a difference of two cumulative sums: absolute, not per element)
    for top_db in (20.0, 40.0, 60.0):
        flags = 10 * np.log10(np.maximum(want, 1e-10)) - 10 * np.log10(max(want.max(), 1e-10)) > -top_db
        if ck.undecided(want, top_db)[0]:
            continue                                                   # the two float64 forms may differ there (none of these inputs does)
        assert np.array_equal(ck.nonsilent(got, top_db), flags)
        idx = np.flatnonzero(flags)
        assert ck.trim(x, top_db) == (512 * idx[0], min(n, 512 * (idx[-1] + 1)))
        iv = ck.split(x, top_db)
        assert iv[0][0] == 512 * idx[0] and iv[-1][1] == min(n, 512 * (idx[-1] + 1))
        assert all(s % 512 == 0 and (e % 512 == 0 or e == n) and flags[s // 512] and flags[(e - 1) // 512] for s, e in iv)
        # the host module's float32 decision on float32-rounded energies agrees outside the band
        f32 = silence.nonsilent(got.astype(np.float32), np.float32(got.max()), top_db)
        assert np.array_equal(f32, flags)
        assert silence.trim_bounds(f32, n) == ck.trim(x, top_db) and silence.split_intervals(f32, n) == iv


def test_frame_counts():
    L = _hip.lib()
    assert L.mcvc_vad_frame_length() == 2048 == silence.FRAME_LENGTH and L.mcvc_vad_hop() == 512 == silence.HOP
    assert L.mcvc_vad_launches() in (1, 2) and L.mcvc_vad_tile_frames() >= 1
    for n, want in ((0, 0), (-5, 0), (1, 1), (511, 1), (512, 2), (1024, 3), (2 ** 31 - 1, 1 + (2 ** 31 - 1) // 512), (2 ** 40, 1 + 2 ** 31)):
        assert L.mcvc_vad_frames(n) == want


@pytest.mark.parametrize("top_db", (40, 60))
def test_golden_trim_bounds(golden_dir, top_db):
    for name, want in GOLDEN_TRIM[top_db].items():
        x = read_wav(os.path.join(golden_dir, "audio", name + ".wav"))
        m = ck.mse(x)
        assert ck.undecided(m, top_db)[0] == 0
        assert ck.trim(x, top_db) == want
        flags = silence.nonsilent(m.astype(np.float32), np.float32(m.max()), top_db)
        assert silence.trim_bounds(flags, x.size) == want
        assert np.allclose(silence.frame_db(m.astype(np.float32), np.float32(m.max())), ck.db(m), atol=1e-5)


def test_symbols_are_declared_exported_and_bound():
    L = _hip.lib()
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcvc.h")) as fh:
        header = fh.read()
    for s in SYMBOLS:
        assert s + "(" in header and s in _hip._SIGS and s in _hip.EXPORTED_SYMBOLS and hasattr(L, s), s
    assert "#define MCVC_ABI_VERSION 3 " in header and L.mcvc_version() == 3
    assert "not verified against librosa" in header


def _plan(offs, max_tiles=None):
    L = _hip.lib()
    offs = np.asarray(offs, dtype=np.int32)
    n = offs.size - 1
    fo = np.full(n + 1, -1, dtype=np.int32)
    nt = ctypes.c_int(-1)
    rc = L.mcvc_vad_plan(offs.ctypes.data, n, fo.ctypes.data, None, 0, ctypes.byref(nt))
    if rc != 0:
        return rc, None, None
    tiles = np.full((nt.value if max_tiles is None else max_tiles, 4), -1, dtype=np.int32)
    nt2 = ctypes.c_int(-1)
    rc = L.mcvc_vad_plan(offs.ctypes.data, n, fo.ctypes.data, tiles.ctypes.data, tiles.shape[0], ctypes.byref(nt2))
    assert nt2.value == nt.value
    return rc, fo, tiles


def test_vad_plan_covers_every_frame_once():
    TF = _hip.lib().mcvc_vad_tile_frames()
    lens = [1, 511, 512, 20001, 512 * TF - 1, 512 * TF, 512 * TF + 1, 1024 * TF + 513, 7]
    offs = np.concatenate([[3], 3 + np.cumsum(lens)])                   # a bank need not start at sample 0
    rc, fo, tiles = _plan(offs)
    assert rc == 0
    T = [ck.frames(n) for n in lens]
    assert np.array_equal(fo, np.concatenate([[0], np.cumsum(T)]))
    cover = np.zeros(fo[-1], dtype=np.int32)
    for s0, n, u, t0 in tiles.tolist():
        assert 0 <= u < len(lens) and s0 == offs[u] and n == lens[u] and t0 % TF == 0 and 0 <= t0 < T[u]
        cover[fo[u] + t0:fo[u] + min(T[u], t0 + TF)] += 1
    assert (cover == 1).all() and tiles.shape[0] == sum(-(-t // TF) for t in T)
    rc, _, short = _plan(offs, max_tiles=tiles.shape[0] - 1)
    assert rc == MCVC_ERR_WORKSPACE and np.array_equal(short, tiles[:-1])


def test_vad_plan_refusals_and_large_indices():
    L = _hip.lib()
    TF = L.mcvc_vad_tile_frames()
    assert _plan([0, 100, 300])[0] == 0
    for offs, why in (([0, 100, 100], "an empty utterance"), ([0, 100, 50], "offsets that fall"), ([-1, 100, 300], "a negative offset")):
        assert _plan(offs)[0] == MCVC_ERR_INVALID, why
    offs = np.array([0, 100, 300], dtype=np.int32)
    fo = np.zeros(3, dtype=np.int32)
    nt = ctypes.c_int(0)
    assert L.mcvc_vad_plan(offs.ctypes.data, 0, fo.ctypes.data, None, 0, ctypes.byref(nt)) == MCVC_ERR_INVALID
    assert L.mcvc_vad_plan(None, 2, fo.ctypes.data, None, 0, ctypes.byref(nt)) == MCVC_ERR_INVALID
    assert L.mcvc_vad_plan(offs.ctypes.data, 2, None, None, 0, ctypes.byref(nt)) == MCVC_ERR_INVALID
    assert L.mcvc_vad_plan(offs.ctypes.data, 2, fo.ctypes.data, None, 0, None) == MCVC_ERR_INVALID
    # the largest bank: one utterance of 2^31 - 1 samples after a short one
    big = [0, 5, 2 ** 31 - 1]
    rc, fo, tiles = _plan(big)
    n = 2 ** 31 - 1 - 5
    assert rc == 0 and fo.tolist() == [0, 1, 1 + ck.frames(n)] and tiles.shape[0] == 1 + -(-ck.frames(n) // TF)
    assert tiles[-1].tolist() == [5, n, 1, (ck.frames(n) - 1) // TF * TF] and tiles[1].tolist() == [5, n, 1, 0]
    # the energy launch refuses before it touches the device: null pointers, a bank of 2^31 samples, misaligned pointers
    a = ctypes.c_void_p(4096)                                           # (never dereferenced: every call below is refused on its arguments)

    def energy(wave=a, n_samples=1000, tiles=a, n_tiles=1, fo=a, n_utts=1, mse=a, total=2, ref=a):
        return L.mcvc_vad_energy(wave, n_samples, tiles, n_tiles, fo, n_utts, mse, total, ref, None)
    for kw in (dict(wave=None), dict(tiles=None), dict(fo=None), dict(mse=None), dict(ref=None), dict(n_samples=0), dict(n_samples=2 ** 31),
               dict(n_tiles=0), dict(n_utts=0), dict(total=0), dict(total=2 ** 31), dict(wave=ctypes.c_void_p(4098)), dict(mse=ctypes.c_void_p(4097)),
               dict(ref=ctypes.c_void_p(4098)), dict(tiles=ctypes.c_void_p(4104)), dict(fo=ctypes.c_void_p(4098))):
        assert energy(**kw) == MCVC_ERR_INVALID, kw


def _audio_plan(offs):
    L = _hip.lib()
    offs = np.asarray(offs, dtype=np.int32)
    n = offs.size - 1
    fo = np.full(n + 1, -1, dtype=np.int32)
    nt = ctypes.c_int(-1)
    assert L.mcvc_audio_plan(offs.ctypes.data, n, fo.ctypes.data, None, 0, ctypes.byref(nt)) == 0
    tiles = np.full((nt.value, 4), -1, dtype=np.int32)
    assert L.mcvc_audio_plan(offs.ctypes.data, n, fo.ctypes.data, tiles.ctypes.data, nt.value, ctypes.byref(nt)) == 0
    return fo, tiles


def _segments(starts, lengths, max_tiles=None):
    L = _hip.lib()
    st, ln = np.asarray(starts, dtype=np.int32), np.asarray(lengths, dtype=np.int32)
    fo = np.full(st.size + 1, -1, dtype=np.int32)
    nt = ctypes.c_int(-1)
    rc = L.mcvc_audio_plan_segments(st.ctypes.data, ln.ctypes.data, st.size, fo.ctypes.data, None, 0, ctypes.byref(nt))
    if rc != 0:
        return rc, None, None
    tiles = np.full((nt.value if max_tiles is None else max_tiles, 4), -1, dtype=np.int32)
    rc = L.mcvc_audio_plan_segments(st.ctypes.data, ln.ctypes.data, st.size, fo.ctypes.data, tiles.ctypes.data, tiles.shape[0], ctypes.byref(nt))
    return rc, fo, tiles


def test_segment_plan_is_the_audio_plan_on_contiguous_segments():
    lens = [385, 20001, 16384, 16385, 57344, 400, 256 * 64 + 128]
    offs = np.concatenate([[0], np.cumsum(lens)])
    fo, tiles = _audio_plan(offs)
    rc, fo2, tiles2 = _segments(offs[:-1], lens)
    assert rc == 0 and fo2.tobytes() == fo.tobytes() and tiles2.tobytes() == tiles.tobytes()


def test_segment_plan_overlapping_and_reordered():
    L = _hip.lib()
    TF = 64
    starts, lens = [50000, 0, 100, 49000], [20000, 385, 40000, 16384 + 256 * 3]
    rc, fo, tiles = _segments(starts, lens)
    assert rc == 0
    T = [L.mcvc_audio_frames(n) for n in lens]
    assert T == [(n - 256) // 256 + 1 for n in lens] and fo.tolist() == np.concatenate([[0], np.cumsum(T)]).tolist()
    want = [[starts[u], lens[u], int(fo[u]) + t0, t0] for u in range(4) for t0 in range(0, T[u], TF)]
    assert tiles.tolist() == want
    rc, _, short = _segments(starts, lens, max_tiles=len(want) - 1)
    assert rc == MCVC_ERR_WORKSPACE and (short == -1).all()            # like mcvc_audio_plan: nothing written


def test_segment_plan_refusals():
    L = _hip.lib()
    assert _segments([0], [385])[0] == 0
    for starts, lens, why in (([0], [384], "under 385 samples"), ([-1], [1000], "a negative start"), ([0, 5], [1000, 0], "an empty segment"),
                              ([2 ** 31 - 1000], [1000], "start + length = 2^31"), ([0], [-5], "a negative length")):
        assert _segments(starts, lens)[0] == MCVC_ERR_INVALID, why
    assert _segments([2 ** 31 - 1001], [1000])[0] == 0                  # start + length = 2^31 - 1: accepted
    st, ln, fo, nt = np.zeros(1, np.int32), np.full(1, 1000, np.int32), np.zeros(2, np.int32), ctypes.c_int(0)
    assert L.mcvc_audio_plan_segments(None, ln.ctypes.data, 1, fo.ctypes.data, None, 0, ctypes.byref(nt)) == MCVC_ERR_INVALID
    assert L.mcvc_audio_plan_segments(st.ctypes.data, None, 1, fo.ctypes.data, None, 0, ctypes.byref(nt)) == MCVC_ERR_INVALID
    assert L.mcvc_audio_plan_segments(st.ctypes.data, ln.ctypes.data, 0, fo.ctypes.data, None, 0, ctypes.byref(nt)) == MCVC_ERR_INVALID
    assert L.mcvc_audio_plan_segments(st.ctypes.data, ln.ctypes.data, 1, None, None, 0, ctypes.byref(nt)) == MCVC_ERR_INVALID
    assert L.mcvc_audio_plan_segments(st.ctypes.data, ln.ctypes.data, 1, fo.ctypes.data, None, 0, None) == MCVC_ERR_INVALID


def test_merge_and_drop_rules():
    G = silence.gap_samples(300.0)
    assert G == 6615 == round(300 * 22.05) and silence.gap_samples(0) == 0
    iv = [(0, 1000), (1000 + G - 1, 30000), (30000 + G, 50000), (50000 + G + 1, 50100), (50100 + 1, 80000)]
    want = [(0, 30000), (30000 + G, 50000), (50000 + G + 1, 80000)]
    for mod in (silence.merge_intervals, ck.merge):
        assert mod(iv, 300.0) == want
        assert mod(iv, 0.0) == iv and mod([], 300.0) == [] and mod(iv, 1e6) == [(0, 80000)]
    # a chain: every gap is measured against the interval as merged so far
    assert silence.merge_intervals([(0, 10), (20, 30), (40, 50)], 1.0) == [(0, 50)] == ck.merge([(0, 10), (20, 30), (40, 50)], 1.0)
    for mod in (silence.drop_short, ck.drop):
        assert mod(want) == ([(0, 30000), (50000 + G + 1, 80000)], 1)          # 13385 samples: dropped; 16384 is kept
        assert mod([(0, 16384), (20000, 36383)]) == ([(0, 16384)], 1) and mod([]) == ([], 0)
    assert silence.MIN_SEGMENT == 16384 == 64 * 256 == preprocess_vcc2018.MIN_FRAMES * 256
    flags = np.array([0, 1, 1, 0, 0, 1, 0, 1], dtype=bool)
    assert silence.split_intervals(flags, 3600) == [(512, 1536), (2560, 3072), (3584, 3600)] == ck.runs(flags, 3600)
    assert silence.trim_bounds(flags, 3600) == (512, 3600)
    for bad in (0, -3.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="top_db"):
            silence.threshold_ratio(bad)
    assert silence.threshold_ratio(40) == np.float32(1e-4) and silence.threshold_ratio(40).dtype == np.float32
    # the decision: strict, clamped at 1e-10 on both sides
    m = np.array([0.0, 1e-12, 1e-4, 1.0, 1.0001e-4], dtype=np.float32)
    assert silence.nonsilent(m, np.float32(1.0), 40).tolist() == [False, False, False, True, True]
    assert silence.nonsilent(np.zeros(3, np.float32), np.float32(0), 40).all()
    assert silence.nonsilent(np.full(3, 1e-12, np.float32), np.float32(1e-12), 40).all()
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            silence.SilenceDetector()


OLD_PREPROCESS = dict(data_directory="w", mel_directory=None, preprocessed_data_directory="vcc2018_preprocessed/vcc2018_training", speaker_ids=["A"],
                      gpu_resample=False)
NEW_TEST = {"trim_silence": None}                                    # (evaluate's namespace is pinned by older tests: its flag leaves no entry when absent)
NEW_PREPROCESS = {"trim_silence": None, "split_silence": None, "min_silence_ms": 300.0}


def _without(cls, new):
    """The parser of ``cls`` as it was before the flags ``new`` existed: the same flag table minus those."""
    p = argparse.ArgumentParser()
    seen = set()
    for klass in reversed(cls.__mro__):
        for flag, kw in klass.__dict__.get("FLAGS", []):
            if flag not in seen and flag[2:] not in new:
                p.add_argument(flag, **kw)
                seen.add(flag)
    for klass in reversed(cls.__mro__):
        if klass.__dict__.get("DEFAULT_OVERRIDES"):
            p.set_defaults(**klass.__dict__["DEFAULT_OVERRIDES"])
    return p


def test_flags_are_off_by_default_and_namespaces_are_todays():
    ns = vars(preprocess_vcc2018.build_parser().parse_args(["--data_directory", "w", "--speaker_ids", "A"]))
    assert ns == dict(OLD_PREPROCESS, **NEW_PREPROCESS)
    t = CycleGANTestArgParser().parser
    t.set_defaults(gl_mel_inverse="pinv", gl_mel_iter=64)
    old = _without(CycleGANTestArgParser, NEW_TEST)
    old.set_defaults(gl_mel_inverse="pinv", gl_mel_iter=64)
    assert vars(t.parse_args([])) == dict(vars(old.parse_args([])), **NEW_TEST)
    argv = ["--target_speaker_id", "T"]
    assert vars(EvaluateArgParser().parse_args(argv)) == vars(_without(EvaluateArgParser, {"trim_silence"}).parse_args(argv))


def test_flag_errors(tmp_path, capsys):
    def refused(call, text):
        with pytest.raises(SystemExit):
            call()
        err = capsys.readouterr().err
        assert text in err, err
    pre = ["--speaker_ids", "A"]
    refused(lambda: preprocess_vcc2018.main(pre + ["--mel_directory", "m", "--trim_silence", "40"]), "--data_directory")
    refused(lambda: preprocess_vcc2018.main(pre + ["--mel_directory", "m", "--split_silence", "40"]), "--data_directory")
    refused(lambda: preprocess_vcc2018.main(pre + ["--data_directory", "w", "--trim_silence", "40", "--split_silence", "40"]), "give one of them")
    refused(lambda: preprocess_vcc2018.main(pre + ["--data_directory", "w", "--trim_silence", "0"]), "finite and > 0")
    refused(lambda: preprocess_vcc2018.main(pre + ["--data_directory", "w", "--split_silence", "-1"]), "finite and > 0")
    refused(lambda: preprocess_vcc2018.main(pre + ["--data_directory", "w", "--split_silence", "nan"]), "finite and > 0")
    refused(lambda: preprocess_vcc2018.main(pre + ["--data_directory", "w", "--split_silence", "40", "--min_silence_ms", "-1"]), "--min_silence_ms")
    ap = preprocess_vcc2018.build_parser()
    a = ap.parse_args(pre + ["--data_directory", "w", "--split_silence", "35", "--min_silence_ms", "150", "--gpu_resample"])
    assert a.split_silence == 35.0 and a.min_silence_ms == 150.0 and a.trim_silence is None and a.gpu_resample
    base = ["--save_dir", str(tmp_path), "--name", "r", "--ckpt_dir", str(tmp_path), "--load_epoch", "1"]
    refused(lambda: CycleGANTestArgParser().parse_args(base + ["--trim_silence", "40"]), "--wav_dir")
    refused(lambda: CycleGANTestArgParser().parse_args(base + ["--wav_dir", "w", "--trim_silence", "inf"]), "finite and > 0")
    a = CycleGANTestArgParser().parse_args(base + ["--wav_dir", "w", "--trim_silence", "40", "--gpu_resample"])
    assert a.trim_silence == 40.0 and a.gpu_resample
    refused(lambda: EvaluateArgParser().parse_args(["--target_speaker_id", "T", "--trim_silence", "40"]), "--target_wav_dir")
    refused(lambda: EvaluateArgParser().parse_args(["--target_wav_dir", "w", "--trim_silence", "0"]), "finite and > 0")
    a = EvaluateArgParser().parse_args(["--target_wav_dir", "w", "--trim_silence", "40", "--f0"])
    assert a.trim_silence == 40.0 and a.f0
    for text in (ap.format_help(), CycleGANTestArgParser().parser.format_help(), EvaluateArgParser().parser.format_help()):
        assert "--trim_silence" in text and "not verified against librosa" in " ".join(text.split())
