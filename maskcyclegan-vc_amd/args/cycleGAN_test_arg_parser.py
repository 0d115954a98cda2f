"""MaskCycleGAN-VC inference flags (reference args/cycleGAN_test_arg_parser.py:16-26)."""
from .base_arg_parser import BaseArgParser


class CycleGANTestArgParser(BaseArgParser):
    isTrain = False
    FLAGS = [
        ("--sample_rate", dict(type=int, default=22050, help="Sampling rate of mel-spectrograms.")),
        ("--speaker_A_id", dict(type=str, default="VCC2SF3", help="Source speaker id (From VOC dataset).")),
        ("--speaker_B_id", dict(type=str, default="VCC2TF1", help="Source speaker id (From VOC dataset).")),
        ("--preprocessed_data_dir", dict(type=str, default="vcc2018_training_preprocessed/", help="Directory containing preprocessed dataset files.")),
        ("--ckpt_dir", dict(type=str, default=None, help="Path to model ckpt.")),
        ("--model_name", dict(type=str, choices=("generator_A2B", "generator_B2A"), default="generator_A2B", help="Name of model to load.")),
        # (new) MI355X inference knobs -- additive, defaults reproduce the reference's fp32 one-utterance-at-a-time results
        ("--dtype", dict(type=str, choices=("f32", "bf16"), default="f32", help="(new) arithmetic of the generator forward: f32 (reference numerics) or bf16 MFMA.")),
        ("--wav_dir", dict(type=str, default=None, help="(new) convert the .wav files of this folder (sorted, recursive) instead of the source speaker's "
                           "preprocessed utterances: mels come from the GPU front-end (data_preprocessing/audio2mel.py) and are standardised with the source "
                           "speaker's norm_stat.npz.  Files not at 22050 Hz are resampled with scipy.signal.resample_poly, which is not librosa's resampler; "
                           "--gpu_resample applies the same filter on the GPU instead.")),
        ("--gpu_resample", dict(action="store_true", help="(new) with --wav_dir: files are read at their own rate and brought to 22050 Hz by the HIP "
                                "polyphase resampler (data_preprocessing/resample.py: scipy's Kaiser-5.0 filter in fp32), one launch per distinct rate.")),
        ("--trim_silence", dict(type=float, default=None, metavar="TOP_DB", help="(new) with --wav_dir: every file is cut to its first .. last "
                                "2048-sample frame within TOP_DB dB of its loudest one before it is converted (data_preprocessing/silence.py: "
                                "librosa.effects.trim restated on the GPU, not verified against librosa).  Default: off.")),
        ("--out_sample_rate", dict(type=int, default=None, metavar="R", help="(new) with --vocoder_ckpt or --griffin_lim: every decoded batch is resampled "
                                   "on the GPU from --sample_rate to R Hz before it is written; the .wav files carry rate R.")),
        ("--vocoder_ckpt", dict(type=str, default=None, help="(new) state dict of the MelGAN vocoder (torch.hub descriptinc/melgan-neurips, saved with "
                                "torch.save): converted and original utterances are also decoded to 32-bit float .wav files under converted_audio/.  "
                                "Without it only converted_mel/*.npy are written.")),
        ("--griffin_lim", dict(type=int, default=0, metavar="N_ITER", help="(new) decode converted and original utterances to 32-bit float .wav files under "
                               "converted_audio/ by N_ITER iterations of Griffin-Lim phase reconstruction on the GPU (mask_cyclegan_vc/griffinlim.py): "
                               "needs no vocoder weights.  0 (default): off.  Not together with --vocoder_ckpt.")),
        ("--gl_mel_inverse", dict(type=str, choices=("pinv", "nnls"), default=None, help="(new) with --griffin_lim: how the 80 mel bands become the 513-bin "
                                  "magnitude the phase loop works on.  pinv (default): the clamped pseudo-inverse.  nnls: non-negative least squares on "
                                  "the GPU (mask_cyclegan_vc/melinv.py), a magnitude whose own mel-spectrogram is the one asked for.")),
        ("--gl_mel_iter", dict(type=int, default=None, metavar="N", help="(new) with --griffin_lim: iterations of the nnls solver, 0 .. 512 (default 64).")),
        ("--max_batch", dict(type=int, default=16, help="(new) utterances of identical length are converted in one batched forward of up to this many.")),
    ]

    def parse_args(self, argv=None):
        self.parser.set_defaults(gl_mel_inverse=None, gl_mel_iter=None)    # None: the flag was not given
        pre = self.parser.parse_args(argv)                             # refused before any run directory is created
        if pre.griffin_lim < 0:
            self.parser.error("--griffin_lim takes a number of iterations >= 0")
        if pre.griffin_lim and pre.vocoder_ckpt:
            self.parser.error("--griffin_lim and --vocoder_ckpt are two decoders for the same files: give one of them")
        if (pre.gl_mel_inverse is not None or pre.gl_mel_iter is not None) and not pre.griffin_lim:
            self.parser.error("--gl_mel_inverse and --gl_mel_iter belong to the Griffin-Lim decoder: give --griffin_lim N_ITER too")
        if pre.out_sample_rate is not None and not (pre.vocoder_ckpt or pre.griffin_lim):
            self.parser.error("--out_sample_rate resamples decoded audio: give --vocoder_ckpt or --griffin_lim N_ITER too")
        if pre.out_sample_rate is not None and pre.out_sample_rate < 1:
            self.parser.error("--out_sample_rate takes a rate in Hz >= 1")
        if pre.gpu_resample and not pre.wav_dir:
            self.parser.error("--gpu_resample resamples the files of --wav_dir: give --wav_dir too")
        if pre.trim_silence is not None:
            from data_preprocessing.preprocess_vcc2018 import check_silence_flags
            check_silence_flags(self.parser, pre, "--wav_dir too", bool(pre.wav_dir))
        if pre.gl_mel_iter is not None and not 0 <= pre.gl_mel_iter <= 512:
            self.parser.error("--gl_mel_iter takes a number of iterations in [0, 512]")
        self.parser.set_defaults(gl_mel_inverse="pinv", gl_mel_iter=64)
        return super(CycleGANTestArgParser, self).parse_args(argv)
