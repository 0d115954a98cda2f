"""Writer of the preprocessed-dataset format the trainer reads (reference data_preprocessing/preprocess_vcc2018.py:26-85).

The reference turns ``.wav`` files into 80-bin mel-spectrograms with the MelGAN vocoder's front-end (``torch.hub``
descriptinc/melgan-neurips + librosa), then standardises per bin over the whole speaker and writes two files:

    <cache>/<spk>/<spk>_normalized.pickle   list of float32 [80, T_i], (mel - mean) / std          (:40-47, :83)
    <cache>/<spk>/<spk>_norm_stat.npz       mean, std: [80, 1]; std = np.std(...) + 1e-9          (:36-38, :78-80)

Utterances shorter than 64 frames are dropped like the reference does (:33).  Two inputs are accepted, exactly one per run:

    --data_directory <dir>   the reference's flag: <dir>/<speaker_id>/**/*.wav.  The wav -> mel step is this project's GPU front-end
                             (data_preprocessing/audio2mel.py: the same fixed transform, one launch per speaker, needs a HIP device).
                             Files that are not at 22050 Hz are resampled with scipy.signal.resample_poly, which is not librosa's
                             resampler; VCC2018 is at 22050 Hz.  --gpu_resample applies the same filter on the GPU instead
                             (data_preprocessing/resample.py), one launch per distinct rate.
                             --trim_silence TOP_DB cuts every file to its first .. last frame within TOP_DB dB of its loudest one;
                             --split_silence TOP_DB [--min_silence_ms 300] makes every non-silent stretch of a long recording an
                             utterance of its own (data_preprocessing/silence.py: librosa.effects.trim / split restated on the GPU, not
                             verified against librosa).  Both are off by default.
    --mel_directory <dir>    <dir>/<speaker_id>/**/*.npy, one [80, T] mel-spectrogram per utterance from any front-end.

    python -m data_preprocessing.preprocess_vcc2018 --data_directory vcc2018/vcc2018_training --preprocessed_data_directory out/ --speaker_ids A B
"""
import argparse
import glob
import os
import pickle

import numpy as np

MIN_FRAMES = 64          # training sample = 64 randomly cropped frames (reference :33)


def normalize_mels(mel_list):
    """-> (list of standardised float32 [80,T_i], mean [80,1], std [80,1]); reference normalize_mel :35-47."""
    mel_list = [np.asarray(m) for m in mel_list if np.asarray(m).shape[-1] >= MIN_FRAMES]
    if not mel_list:
        raise ValueError("no utterance has >= %d frames" % MIN_FRAMES)
    cat = np.concatenate(mel_list, axis=1)
    mean = np.mean(cat, axis=1, keepdims=True)
    std = np.std(cat, axis=1, keepdims=True) + 1e-9
    return [((m - mean) / std).astype(np.float32) for m in mel_list], mean, std


def save_preprocessed(cache_folder, speaker_id, mel_list):
    """Standardise and write the two files of one speaker (reference preprocess_dataset :62-85)."""
    normalized, mean, std = normalize_mels(mel_list)
    d = os.path.join(cache_folder, speaker_id)
    os.makedirs(d, exist_ok=True)
    np.savez(os.path.join(d, "%s_norm_stat.npz" % speaker_id), mean=mean, std=std)
    with open(os.path.join(d, "%s_normalized.pickle" % speaker_id), "wb") as fh:
        pickle.dump(normalized, fh)
    return d


def speaker_mels_from_wavs(data_directory, speaker_id, fft=None, gpu_resample=False, trim_db=None, split_db=None, min_silence_ms=300.0, report=None):
    """Sorted <dir>/<spk>/**/*.wav -> (files, list of float32 [80, T_i]): one bank launch for the whole speaker.  ``gpu_resample``: files
    are read at their own rate and brought to 22050 Hz on the device (``Audio2Mel.bank_at_rates``) instead of by scipy on the host.
    ``trim_db``: every file is trimmed to its non-silent span.  ``split_db``: every kept non-silent interval of a file is an utterance, in
    file order and then time order; ``report`` (a dict) then receives the counts ``main`` prints."""
    from .audio2mel import Audio2Mel, read_wav, read_wav_native
    files = sorted(glob.glob(os.path.join(data_directory, speaker_id, "**", "*.wav"), recursive=True))
    if not files:
        raise ValueError("no .wav files under %s" % os.path.join(data_directory, speaker_id))
    fft = fft or Audio2Mel()
    if split_db is not None:
        native = [read_wav_native(f) for f in files] if gpu_resample else [(None, read_wav(f)) for f in files]
        mels, intervals, _, stats = fft.bank_split([x for _, x in native], split_db, min_silence_ms, rates=[r for r, _ in native] if gpu_resample else None,
                                                   return_segments=True)
        if report is not None:
            report.update(files=len(files), utterances=len(mels), dropped=int(sum(stats["dropped"])),
                          kept_share=sum(e - s for s, e in intervals) / float(max(1, sum(stats["samples"]))))
        return files, mels
    if trim_db is not None:
        if gpu_resample:
            native = [read_wav_native(f) for f in files]
            return files, fft.bank_at_rates([x for _, x in native], [r for r, _ in native], trim_db=trim_db)
        return files, fft.bank([read_wav(f) for f in files], trim_db=trim_db)
    if gpu_resample:
        native = [read_wav_native(f) for f in files]
        return files, fft.bank_at_rates([x for _, x in native], [r for r, _ in native])
    return files, fft.bank([read_wav(f) for f in files])


def build_parser():
    ap = argparse.ArgumentParser(description=".wav files (or mel-spectrogram .npy files) -> preprocessed speaker folders")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--data_directory", type=str, default=None,
                     help="<dir>/<speaker_id>/**/*.wav (the reference's flag); mels are computed on the GPU.  Files not at 22050 Hz are "
                          "resampled with scipy.signal.resample_poly, which is not librosa's resampler; --gpu_resample applies the same filter "
                          "on the GPU instead.")
    src.add_argument("--mel_directory", type=str, default=None, help="<dir>/<speaker_id>/**/*.npy, one [80,T] array per utterance")
    ap.add_argument("--preprocessed_data_directory", type=str, default="vcc2018_preprocessed/vcc2018_training")
    ap.add_argument("--speaker_ids", nargs="+", type=str, required=True)
    ap.add_argument("--gpu_resample", action="store_true",
                    help="with --data_directory: files are read at their own rate and brought to 22050 Hz by the HIP polyphase resampler "
                         "(data_preprocessing/resample.py: scipy's Kaiser-5.0 filter in fp32)")
    ap.add_argument("--trim_silence", type=float, default=None, metavar="TOP_DB",
                    help="with --data_directory: every file is cut to its first .. last 2048-sample frame within TOP_DB dB of its loudest one "
                         "(data_preprocessing/silence.py: librosa.effects.trim restated on the GPU, not verified against librosa).  40 suits "
                         "studio clips like VCC2018.  Default: off.")
    ap.add_argument("--split_silence", type=float, default=None, metavar="TOP_DB",
                    help="with --data_directory: every non-silent stretch of a file (librosa.effects.split restated, same frames and threshold) "
                         "becomes an utterance of its own, in file order and then time order; stretches under 64 mel frames are dropped.  "
                         "Not together with --trim_silence.  Default: off.")
    ap.add_argument("--min_silence_ms", type=float, default=300.0, metavar="MS",
                    help="with --split_silence: stretches closer than this many milliseconds are joined (default 300)")
    return ap


def check_silence_flags(ap, args, wav_flag, have_wavs):
    """The parser errors the commands with --trim_silence share."""
    from .silence import gap_samples, threshold_ratio
    for flag in ("trim_silence", "split_silence"):
        v = getattr(args, flag, None)
        if v is None:
            continue
        if not have_wavs:
            ap.error("--%s works on .wav files: give %s" % (flag, wav_flag))
        try:
            threshold_ratio(v)
        except ValueError:
            ap.error("--%s takes a level in dB below the loudest frame, finite and > 0" % flag)
    if getattr(args, "split_silence", None) is not None and args.trim_silence is not None:
        ap.error("--trim_silence and --split_silence are two ways to cut the same files: give one of them")
    if getattr(args, "split_silence", None) is not None:
        try:
            gap_samples(args.min_silence_ms)
        except ValueError:
            ap.error("--min_silence_ms takes a duration in milliseconds, finite and >= 0")


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.gpu_resample and args.data_directory is None:
        ap.error("--gpu_resample resamples .wav files: give --data_directory")
    check_silence_flags(ap, args, "--data_directory", args.data_directory is not None)
    fft = None
    for spk in args.speaker_ids:
        if args.data_directory is not None:
            if fft is None:
                from .audio2mel import Audio2Mel
                fft = Audio2Mel()
            if args.trim_silence is None and args.split_silence is None:
                files, mels = speaker_mels_from_wavs(args.data_directory, spk, fft, args.gpu_resample)
            else:
                report = {}
                files, mels = speaker_mels_from_wavs(args.data_directory, spk, fft, args.gpu_resample, args.trim_silence, args.split_silence,
                                                     args.min_silence_ms, report)
                if report:
                    print("Split on silence for speaker: %s (%d files -> %d utterances, %d intervals dropped as shorter than %d frames, %.1f %% of "
                          "the samples kept)" % (spk, report["files"], report["utterances"], report["dropped"], MIN_FRAMES, 100.0 * report["kept_share"]))
        else:
            files = sorted(glob.glob(os.path.join(args.mel_directory, spk, "**", "*.npy"), recursive=True))
            mels = [np.load(f) for f in files]
        d = save_preprocessed(args.preprocessed_data_directory, spk, mels)
        print("Preprocessed and saved data for speaker: %s (%d files) -> %s" % (spk, len(files), d))


if __name__ == "__main__":
    main()
