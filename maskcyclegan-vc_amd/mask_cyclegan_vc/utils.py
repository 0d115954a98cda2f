"""Vocoder / figure helpers of the reference (mask_cyclegan_vc/utils.py:25-65).

``decode_melspectrogram`` is the reference's own two lines (utils.py:37-39) on the HIP MelGAN decoder (``vocoder`` is a
``mask_cyclegan_vc.vocoder.MelVocoder``; any object with the hub model's ``inverse`` works).  ``get_mel_spectrogram_fig`` needs
matplotlib / librosa / cv2, none of which are on the hot path: the name exists so reference-style imports
resolve, and calling it explains what to do."""


def _out_of_scope(name):
    raise NotImplementedError(
        "%s needs plotting packages (matplotlib, librosa, cv2) that are not part of the MI355X hot-path build; the converted "
        "mel-spectrograms are written as .npy (see test.py) and can be plotted from there" % name)


def decode_melspectrogram(vocoder, melspectrogram, mel_mean, mel_std):
    """[80, T] standardised mel -> [1, 256 T] waveform (reference utils.py:37-39).  ``vocoder`` is any object with an ``inverse``
    that takes a [B, 80, T] log10-mel: ``vocoder.MelVocoder`` (trained weights) or ``griffinlim.GriffinLimVocoder`` (none needed)."""
    denorm_converted = melspectrogram * mel_std + mel_mean
    rev = vocoder.inverse(denorm_converted.unsqueeze(0))
    return rev


def get_mel_spectrogram_fig(spec, title="Mel-Spectrogram"):
    _out_of_scope("get_mel_spectrogram_fig")


def denormalize_mel(mel, mel_mean, mel_std):
    """The numeric half of the reference's decode (utils.py:36): undo the per-bin standardisation."""
    return mel * mel_std + mel_mean
