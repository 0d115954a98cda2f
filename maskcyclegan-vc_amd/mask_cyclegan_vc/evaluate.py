"""``python -m mask_cyclegan_vc.evaluate`` -- how good is the conversion: mel-cepstral distortion (MCD, dB) after dynamic-time-warping
alignment of every converted utterance against the target speaker's recording of the same sentence (mask_cyclegan_vc/metrics.py; the
arithmetic runs in csrc/dtw_kernels.hip).  New: the reference has no objective evaluation.

Inputs: the ``converted_mel/`` folder ``mask_cyclegan_vc.test`` writes (``<i>-converted_<src>_to_<tgt>.npy``, i = index in the source
list) and the references, from one of

* ``--preprocessed_data_dir`` + ``--target_speaker_id``: the target speaker's preprocessed cache, de-normalised with its norm_stat;
* ``--target_wav_dir``: the folder's sorted .wav files through ``Audio2Mel``.  ``--trim_silence TOP_DB`` (with this input only) first cuts
  every recording to its first .. last frame within TOP_DB dB of its loudest one (data_preprocessing/silence.py): the same bounds cut what
  the mel bank and what the ``--f0`` tracker see, and ``metrics.json`` gains ``"trim_silence_db"``.

Reference i must be the same sentence as source utterance i (VCC2018 is a parallel corpus; its sorted file lists line up).  That is the
caller's contract: nothing here can check it.  An index without a reference is an error.  ``--source_speaker_id`` adds the unconverted
baseline (source against target), the usual second column.

Output: ``<save_dir>/<name>/metrics.json`` (per utterance: MCD, path length, frames of both sides; mean, std, median; n_cep; the baseline
if asked) and one printed summary line.  The cepstra come from the 80-band mel spectrum, not from WORLD: the numbers compare runs of this
project, not tables in papers.

``--f0`` (needs ``--target_wav_dir``) adds the pitch columns: F0 RMSE and bias in cents and the voiced/unvoiced error along the same DTW
alignment (mask_cyclegan_vc/pitch.py, metrics.f0_distortion), from the ``<i>-converted_*.wav`` files of ``--converted_audio_dir`` (default
``<save_dir>/<name>/converted_audio``, what ``mask_cyclegan_vc.test`` writes with a decoder) and the target recordings.  Without the flag the
run and its ``metrics.json`` are what they were.

``--msd`` adds an ``"msd"`` object: the modulation-spectrum distance and the global-variance distance (dB) of ALL converted utterances
against ALL utterances of the target speaker (metrics.msd; ``--msd_n_fft``, ``--msd_max_hz``).  The two sets are not index-matched and need
not be parallel.  ``target_split_half_msd`` scores the target's even-indexed against its odd-indexed utterances: the floor a perfect
conversion would reach (null with fewer than two).  With ``--source_speaker_id`` the unconverted source gives ``baseline_msd`` /
``baseline_gvd``.  ``--no_mcd`` (with ``--msd``, not with ``--f0``) serves a corpus without parallel sentences: no MCD, no baseline MCD, no
index contract; the report then holds ``n_utterances``, per utterance ``index``, ``file`` and ``frames_converted``, and the ``msd`` object."""
import glob
import json
import os
import re

import numpy as np

from args.evaluate_arg_parser import EvaluateArgParser

from . import metrics
from .utils import denormalize_mel

_NAME = re.compile(r"^(\d+)-converted_.*\.npy$")
_WAV_NAME = re.compile(r"^(\d+)-converted_.*\.wav$")
F0_UNIT = ("cents = 1200 log2(f0 converted / f0 target) over the DTW path rows where both sides are voiced; vuv_error = path rows where exactly one "
           "side is voiced / path length; YIN on decoded audio (not WORLD / Harvest)")


def converted_files(folder):
    """-> sorted [(i, path)] of the folder's <i>-converted_*.npy files."""
    found = []
    for p in glob.glob(os.path.join(folder, "*.npy")):
        m = _NAME.match(os.path.basename(p))
        if m:
            found.append((int(m.group(1)), p))
    if not found:
        raise ValueError("no <i>-converted_*.npy files under %s" % folder)
    found.sort()
    ids = [i for i, _ in found]
    if len(set(ids)) != len(ids):
        raise ValueError("%s holds several files for one utterance index (two conversions in one folder?)" % folder)
    return found


def speaker_mels(preprocessed_dir, speaker_id):
    """The speaker's preprocessed utterances, de-normalised: list of float32 [80, T]."""
    from .train import load_speaker
    mels, mean, std = load_speaker(preprocessed_dir, speaker_id)
    return [denormalize_mel(np.asarray(m, dtype=np.float32), mean, std).astype(np.float32) for m in mels]


def wav_dir_waves(folder):
    from data_preprocessing.audio2mel import read_wav
    files = sorted(glob.glob(os.path.join(folder, "**", "*.wav"), recursive=True))
    if not files:
        raise ValueError("no .wav files under %s" % folder)
    return [read_wav(f) for f in files]


def converted_waves(folder, ids):
    """The <i>-converted_*.wav of every index in ``ids`` -> list of float32 waveforms."""
    from data_preprocessing.audio2mel import read_wav
    found = {}
    for p in sorted(glob.glob(os.path.join(folder, "*.wav"))):
        m = _WAV_NAME.match(os.path.basename(p))
        if m:
            if int(m.group(1)) in found:
                raise ValueError("%s holds several .wav files for one utterance index (two conversions in one folder?)" % folder)
            found[int(m.group(1))] = p
    for i in ids:
        if i not in found:
            raise ValueError("converted utterance %d has no converted audio: no %d-converted_*.wav under %s (mask_cyclegan_vc.test writes them "
                             "with --vocoder_ckpt or --griffin_lim)" % (i, i, folder))
    return [read_wav(found[i]) for i in ids]


def _voiced_median(tracks):
    v = np.concatenate([t[t > 0] for t in tracks]) if tracks else np.zeros(0)
    return float(np.median(v)) if v.size else None


MSD_UNIT = ("dB; root mean square difference of the two sets' mean log modulation spectra (msd) / mean log global variances (gvd) of mel-cepstra "
            "from the 80-band log-mel (not WORLD) at 86.13 frames per second (not 200): compares runs of this project, not tables in papers")


def msd_report(args, converted, refs, source=None):
    """The ``"msd"`` object of the report: all converted against all target utterances."""
    res = metrics.msd(converted, refs, args.n_cep, args.msd_n_fft, args.msd_max_hz)
    out = {"msd": res["msd"], "gvd": res["gvd"], "msd_per_dim": [float(v) for v in res["msd_per_dim"]],
           "lgv_converted": [float(v) for v in res["lgv_converted"]], "lgv_target": [float(v) for v in res["lgv_target"]],
           "n_converted": res["n_converted"], "n_target": res["n_target"], "n_fft": res["n_fft"], "max_hz": res["max_hz"], "floor": res["floor"],
           "unit": MSD_UNIT, "target_split_half_msd": None}
    if len(refs) >= 2:
        out["target_split_half_msd"] = metrics.msd(refs[0::2], refs[1::2], args.n_cep, args.msd_n_fft, args.msd_max_hz)["msd"]
    if source is not None:
        base = metrics.msd(source, refs, args.n_cep, args.msd_n_fft, args.msd_max_hz)
        out.update(baseline_msd=base["msd"], baseline_gvd=base["gvd"])
    return out


def _msd_clause(m):
    line = "MSD %.3f dB, GVD %.3f dB (%d converted against %d target utterances, n_fft %d" % (m["msd"], m["gvd"], m["n_converted"], m["n_target"], m["n_fft"])
    if m["target_split_half_msd"] is not None:
        line += "; target split-half MSD %.3f dB" % m["target_split_half_msd"]
    if "baseline_msd" in m:
        line += "; unconverted baseline MSD %.3f dB, GVD %.3f dB" % (m["baseline_msd"], m["baseline_gvd"])
    return line + ")"


def _pick(refs, ids, what):
    for i in ids:
        if i >= len(refs):
            raise ValueError("converted utterance %d has no %s: only %d are there (indices 0 .. %d); reference i must be the recording of "
                             "the sentence of source utterance i" % (i, what, len(refs), len(refs) - 1))
    return [refs[i] for i in ids]


def _stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"mean": float(v.mean()), "std": float(v.std()), "median": float(np.median(v))}


def evaluate(args):
    run_dir = os.path.join(args.save_dir, args.name)
    files = converted_files(args.converted_dir or os.path.join(run_dir, "converted_mel"))
    ids = [i for i, _ in files]
    converted = [np.load(p).astype(np.float32) for _, p in files]
    trim_db = getattr(args, "trim_silence", None)                      # (absent unless the flag was given)
    if args.target_wav_dir:
        from data_preprocessing.audio2mel import Audio2Mel
        ref_waves = wav_dir_waves(args.target_wav_dir)
        if trim_db is not None:                                         # one set of bounds for the mel bank and the F0 tracker
            refs, bounds = Audio2Mel().bank(ref_waves, trim_db=trim_db, return_bounds=True)
            ref_waves = [w[s:e] for w, (s, e) in zip(ref_waves, bounds)]
        else:
            refs = Audio2Mel().bank(ref_waves)
    else:
        refs = speaker_mels(args.preprocessed_data_dir, args.target_speaker_id)
    if args.no_mcd:
        source = _pick(speaker_mels(args.preprocessed_data_dir, args.source_speaker_id), ids, "source utterance") if args.source_speaker_id else None
        utts = [{"index": i, "file": os.path.basename(p), "frames_converted": int(converted[k].shape[1])} for k, (i, p) in enumerate(files)]
        report = {"n_cep": int(args.n_cep), "n_utterances": len(utts), "utterances": utts, "msd": msd_report(args, converted, refs, source)}
        if trim_db is not None:
            report["trim_silence_db"] = float(trim_db)
        os.makedirs(run_dir, exist_ok=True)
        out = os.path.join(run_dir, "metrics.json")
        with open(out, "w") as fh:
            json.dump(report, fh, indent=2)
        print(_msd_clause(report["msd"]) + " -> " + out)
        return report
    target = _pick(refs, ids, "reference")
    res = metrics.mcd(converted, target, args.n_cep)
    base = None
    if args.source_speaker_id:
        source = _pick(speaker_mels(args.preprocessed_data_dir, args.source_speaker_id), ids, "source utterance")
        base = metrics.mcd(source, target, args.n_cep)
    utts = []
    for k, (i, p) in enumerate(files):
        u = {"index": i, "file": os.path.basename(p), "mcd": float(res["mcd"][k]), "length": int(res["length"][k]),
             "frames_converted": int(res["frames_converted"][k]), "frames_target": int(res["frames_target"][k])}
        if base is not None:
            u.update(baseline_mcd=float(base["mcd"][k]), baseline_length=int(base["length"][k]), frames_source=int(base["frames_converted"][k]))
        utts.append(u)
    report = {"n_cep": int(args.n_cep), "n_utterances": len(utts), "unit": "dB, mean over the DTW path; cepstra from the 80-band log-mel (not WORLD)",
              "utterances": utts}
    report.update(_stats(res["mcd"]))
    if base is not None:
        report["baseline"] = _stats(base["mcd"])
    if args.f0:
        from .pitch import PitchTracker
        tracker = PitchTracker(fmin=args.f0_min, fmax=args.f0_max, threshold=args.f0_threshold)
        f0 = metrics.f0_distortion(converted_waves(args.converted_audio_dir or os.path.join(run_dir, "converted_audio"), ids),
                                   _pick(ref_waves, ids, "reference"), converted, target, args.n_cep, tracker)
        for k, u in enumerate(utts):
            some = int(f0["voiced_pairs"][k]) > 0                       # (a pair without a both-voiced row has no cent figures: null)
            u.update(f0_rmse_cents=float(f0["rmse_cents"][k]) if some else None, f0_bias_cents=float(f0["bias_cents"][k]) if some else None,
                     vuv_error=float(f0["vuv_error"][k]), voiced_pairs=int(f0["voiced_pairs"][k]))
        keep = f0["voiced_pairs"] > 0
        report["f0"] = {"n_utterances_voiced": int(keep.sum()), "tau_min": int(tracker.lags[0]), "tau_max": int(tracker.lags[1]),
                        "f0_min": float(args.f0_min), "f0_max": float(args.f0_max), "threshold": float(tracker.threshold),
                        "median_f0_converted_hz": _voiced_median(f0["f0_converted"]), "median_f0_target_hz": _voiced_median(f0["f0_target"]),
                        "unit": F0_UNIT}
        for key in ("rmse_cents", "bias_cents", "vuv_error"):
            report["f0"][key] = _stats(f0[key][keep]) if keep.any() else None
    if args.msd:
        report["msd"] = msd_report(args, converted, refs, source if base is not None else None)
    if trim_db is not None:
        report["trim_silence_db"] = float(trim_db)
    os.makedirs(run_dir, exist_ok=True)
    out = os.path.join(run_dir, "metrics.json")
    with open(out, "w") as fh:
        json.dump(report, fh, indent=2)
    line = "MCD over %d utterances (n_cep %d): mean %.3f dB, std %.3f, median %.3f" % (len(utts), args.n_cep, report["mean"], report["std"], report["median"])
    if base is not None:
        line += " | unconverted baseline: mean %.3f dB" % report["baseline"]["mean"]
    if args.f0 and report["f0"]["rmse_cents"] is not None:
        line += " | F0 RMSE %.1f cents, bias %+.1f cents, V/UV error %.1f %% (%d utterances with voiced pairs)" % (
            report["f0"]["rmse_cents"]["mean"], report["f0"]["bias_cents"]["mean"], 100.0 * report["f0"]["vuv_error"]["mean"], report["f0"]["n_utterances_voiced"])
    elif args.f0:
        line += " | F0: no utterance with a voiced pair"
    if args.msd:
        line += " | " + _msd_clause(report["msd"])
    print(line + " -> " + out)
    return report


def main(argv=None):
    return evaluate(EvaluateArgParser().parse_args(argv))


if __name__ == "__main__":
    main()
