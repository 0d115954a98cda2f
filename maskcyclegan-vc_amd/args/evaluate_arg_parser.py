"""Flags of ``python -m mask_cyclegan_vc.evaluate`` (new: the reference has no objective evaluation).  A plain parser: evaluation seeds
nothing, loads no checkpoint and creates nothing but ``metrics.json`` in the run directory."""
import argparse


class EvaluateArgParser(object):
    FLAGS = [
        ("--name", dict(type=str, default="debug", help="Experiment name: the run directory is <save_dir>/<name>, as for mask_cyclegan_vc.test.")),
        ("--save_dir", dict(type=str, default="/home/results/", help="Directory for results.")),
        ("--converted_dir", dict(type=str, default=None, help="Folder of <i>-converted_<src>_to_<tgt>.npy files as mask_cyclegan_vc.test writes them "
                                 "(i: index in the source list).  Default: <save_dir>/<name>/converted_mel.")),
        ("--preprocessed_data_dir", dict(type=str, default="vcc2018_training_preprocessed/", help="Directory containing preprocessed dataset files.")),
        ("--target_speaker_id", dict(type=str, default=None, help="References: the target speaker's preprocessed cache, de-normalised with its norm_stat. "
                                     "Utterance i must be the sentence of converted utterance i (a parallel corpus): that is the caller's contract.")),
        ("--target_wav_dir", dict(type=str, default=None, help="References: the sorted .wav files of this folder through the GPU front-end "
                                  "(data_preprocessing/audio2mel.py).  File i must be the sentence of converted utterance i.")),
        ("--source_speaker_id", dict(type=str, default=None, help="Also report the unconverted baseline: the source speaker's preprocessed utterances "
                                     "against the same references.")),
        ("--n_cep", dict(type=int, default=24, help="Mel-cepstral coefficients c_1 .. c_n_cep (1 .. 79) from the 80-band log-mel.")),
        ("--f0", dict(action="store_true", help="Also report F0 RMSE / bias in cents and the voiced/unvoiced error along the same DTW alignment: "
                      "YIN on the GPU (mask_cyclegan_vc/pitch.py) over the converted .wav files and the target recordings.  Needs --target_wav_dir "
                      "(preprocessed caches hold no audio).")),
        ("--converted_audio_dir", dict(type=str, default=None, help="With --f0: folder of <i>-converted_<src>_to_<tgt>.wav files as mask_cyclegan_vc.test "
                                       "writes them with a decoder.  Default: <save_dir>/<name>/converted_audio.")),
        ("--f0_min", dict(type=float, default=60.0, help="With --f0: lowest F0 searched, Hz (longest lag floor(22050 / f0_min) <= 640).")),
        ("--f0_max", dict(type=float, default=500.0, help="With --f0: highest F0 searched, Hz (shortest lag ceil(22050 / f0_max) >= 2).")),
        ("--f0_threshold", dict(type=float, default=0.15, help="With --f0: YIN's threshold on the normalised difference function, in (0, 1].")),
        ("--trim_silence", dict(type=float, default=argparse.SUPPRESS, metavar="TOP_DB", help="With --target_wav_dir: the target recordings are cut to their first "
                                ".. last 2048-sample frame within TOP_DB dB of their loudest one (data_preprocessing/silence.py: librosa.effects.trim "
                                "restated on the GPU, not verified against librosa) before the mel bank and the --f0 tracker see them.  Default: off (the "
                                "parsed arguments then carry no such entry).")),
        ("--msd", dict(action="store_true", help="Also report the modulation-spectrum distance (MSD) and the global-variance distance (GVD), in dB, of "
                       "ALL converted utterances against ALL of the target speaker's: two sets, no alignment, no parallel sentences needed "
                       "(mask_cyclegan_vc/metrics.py msd).")),
        ("--msd_n_fft", dict(type=int, default=4096, choices=(1024, 2048, 4096), help="With --msd: length the mean-removed cepstral trajectories are "
                             "zero-padded to; no utterance may be longer.")),
        ("--msd_max_hz", dict(type=float, default=None, help="With --msd: compare the modulation bins at or below this frequency only "
                              "(default: all, up to Nyquist = 43.07 Hz).")),
        ("--no_mcd", dict(action="store_true", help="For a corpus without parallel sentences: skip MCD, its baseline and the rule that reference i is the "
                          "sentence of converted utterance i.  Needs --msd; not with --f0.")),
    ]

    def __init__(self):
        self.parser = argparse.ArgumentParser(description=type(self).__name__)
        for flag, kw in self.FLAGS:
            self.parser.add_argument(flag, **kw)

    def parse_args(self, argv=None):
        args = self.parser.parse_args(argv)
        if (args.target_speaker_id is None) == (args.target_wav_dir is None):
            self.parser.error("give the references as exactly one of --target_speaker_id and --target_wav_dir")
        if not 1 <= args.n_cep <= 79:
            self.parser.error("--n_cep takes a number of coefficients in 1 .. 79")
        if args.f0 and args.target_wav_dir is None:
            self.parser.error("--f0 needs the references as audio: give --target_wav_dir (preprocessed caches hold no waveforms)")
        if getattr(args, "trim_silence", None) is not None:
            from data_preprocessing.preprocess_vcc2018 import check_silence_flags
            check_silence_flags(self.parser, args, "--target_wav_dir", args.target_wav_dir is not None)
        if args.no_mcd and not args.msd:
            self.parser.error("--no_mcd leaves nothing to report: give --msd with it")
        if args.no_mcd and args.f0:
            self.parser.error("--f0 runs along the DTW alignment that --no_mcd skips: give one of the two")
        if args.msd_max_hz is not None:
            from mask_cyclegan_vc.metrics import ms_bins
            try:
                ms_bins(args.msd_n_fft, args.msd_max_hz)
            except ValueError as exc:
                self.parser.error("--msd_max_hz: %s" % exc)
        from mask_cyclegan_vc.pitch import check_threshold, lag_range
        try:
            lag_range(args.f0_min, args.f0_max)
            check_threshold(args.f0_threshold)
        except ValueError as exc:
            self.parser.error(str(exc))
        return args
