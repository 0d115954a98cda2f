"""``python -m mask_cyclegan_vc.evaluate`` -- how good is the conversion: mel-cepstral distortion (MCD, dB) after dynamic-time-warping
alignment of every converted utterance against the target speaker's recording of the same sentence (mask_cyclegan_vc/metrics.py; the
arithmetic runs in csrc/dtw_kernels.hip).  New: the reference has no objective evaluation.

Inputs: the ``converted_mel/`` folder ``mask_cyclegan_vc.test`` writes (``<i>-converted_<src>_to_<tgt>.npy``, i = index in the source
list) and the references, from one of

* ``--preprocessed_data_dir`` + ``--target_speaker_id``: the target speaker's preprocessed cache, de-normalised with its norm_stat;
* ``--target_wav_dir``: the folder's sorted .wav files through ``Audio2Mel``.

Reference i must be the same sentence as source utterance i (VCC2018 is a parallel corpus; its sorted file lists line up).  That is the
caller's contract: nothing here can check it.  An index without a reference is an error.  ``--source_speaker_id`` adds the unconverted
baseline (source against target), the usual second column.

Output: ``<save_dir>/<name>/metrics.json`` (per utterance: MCD, path length, frames of both sides; mean, std, median; n_cep; the baseline
if asked) and one printed summary line.  The cepstra come from the 80-band mel spectrum, not from WORLD: the numbers compare runs of this
project, not tables in papers."""
import glob
import json
import os
import re

import numpy as np

from args.evaluate_arg_parser import EvaluateArgParser

from . import metrics
from .utils import denormalize_mel

_NAME = re.compile(r"^(\d+)-converted_.*\.npy$")


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


def wav_dir_mels(folder):
    from data_preprocessing.audio2mel import Audio2Mel, read_wav
    files = sorted(glob.glob(os.path.join(folder, "**", "*.wav"), recursive=True))
    if not files:
        raise ValueError("no .wav files under %s" % folder)
    return Audio2Mel().bank([read_wav(f) for f in files])


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
    if args.target_wav_dir:
        refs = wav_dir_mels(args.target_wav_dir)
    else:
        refs = speaker_mels(args.preprocessed_data_dir, args.target_speaker_id)
    target = _pick(refs, ids, "reference")
    res = metrics.mcd(converted, target, args.n_cep)
    base = None
    if args.source_speaker_id:
        base = metrics.mcd(_pick(speaker_mels(args.preprocessed_data_dir, args.source_speaker_id), ids, "source utterance"), target, args.n_cep)
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
    os.makedirs(run_dir, exist_ok=True)
    out = os.path.join(run_dir, "metrics.json")
    with open(out, "w") as fh:
        json.dump(report, fh, indent=2)
    line = "MCD over %d utterances (n_cep %d): mean %.3f dB, std %.3f, median %.3f" % (len(utts), args.n_cep, report["mean"], report["std"], report["median"])
    if base is not None:
        line += " | unconverted baseline: mean %.3f dB" % report["baseline"]["mean"]
    print(line + " -> " + out)
    return report


def main(argv=None):
    return evaluate(EvaluateArgParser().parse_args(argv))


if __name__ == "__main__":
    main()
