"""``python -m mask_cyclegan_vc.test`` -- drop-in for the reference inference driver (mask_cyclegan_vc/test.py:18-126).

Loads one generator checkpoint and converts every utterance of the source speaker with an all-ones mask
(test.py:92, 107).  The converted, de-normalised mel-spectrograms are always written as .npy under converted_mel/.

``--vocoder_ckpt`` (new): the reference's last step (test.py:94-103).  The MelGAN weights cannot be fetched by this build, so the
user supplies the hub model's state dict; with it every converted utterance and its de-normalised source are decoded by the HIP MelGAN
decoder (mask_cyclegan_vc/vocoder.py; one batched ``inverse`` each per bucket, on the bucket's stream) and written under
converted_audio/ with the reference's file names, as 32-bit float WAV at ``--sample_rate`` (what torchaudio.save writes for a float
tensor).  The decoder reads exactly the float32 values the .npy files hold.

Batching (new): InstanceNorm statistics run over an utterance's whole time axis, so zero-padding utterances to a common
length would change every output.  Utterances are therefore bucketed by EXACT length: a bucket of k equal-length utterances
is one batched forward (up to ``--max_batch``; every op is per-sample, so results equal the bs=1 results), buckets are
visited longest first and alternate between two HIP streams so that short utterances overlap on the chip.  ``--dtype bf16``
selects the bf16-MFMA forward (BASELINE configs[4]).

``--griffin_lim N_ITER`` (new): the same two files per utterance without any vocoder weights -- N_ITER iterations of Griffin-Lim phase
reconstruction against the front-end's own STFT (mask_cyclegan_vc/griffinlim.py, csrc/griffinlim_kernels.hip), through the same
``write_audio`` path.  Not together with ``--vocoder_ckpt``; with neither flag no audio is written and neither decoder is imported.
``--gl_mel_inverse nnls`` (new, with ``--griffin_lim`` only; ``--gl_mel_iter N``, default 64): the magnitude the phase loop works on
comes from the non-negative least-squares solver of mask_cyclegan_vc/melinv.py instead of the clamped pseudo-inverse; the default
``pinv`` writes the files it always wrote.

``--wav_dir`` (new): the utterances to convert are the .wav files of a folder instead of the source speaker's pickle; their
mel-spectrograms come from the GPU front-end (data_preprocessing/audio2mel.py).  ``--gpu_resample`` (new): files that are not at
22050 Hz are resampled by the HIP polyphase kernel (data_preprocessing/resample.py) instead of scipy on the host.
``--trim_silence TOP_DB`` (new, with ``--wav_dir``): every file is cut to its first .. last frame within TOP_DB dB of its loudest one
before it is converted (data_preprocessing/silence.py; the mels of the trimmed spans come from the same uploaded bank).

``--out_sample_rate R`` (new, with a decoder only): each decoded batch [B, 256 T] is resampled on its bucket's stream from
``--sample_rate`` to R Hz before the copy to the host; the files carry rate R and ceil(256 T up / down) samples."""
import os

import numpy as np
import torch

from args.cycleGAN_test_arg_parser import CycleGANTestArgParser
from saver.model_saver import ModelSaver

from .model import Generator
from .train import load_speaker
from .utils import denormalize_mel


class MaskCycleGANVCTesting(object):
    def __init__(self, args):
        self.args = args
        if not torch.cuda.is_available():
            raise RuntimeError("mask_cyclegan_vc.test (MI355X build) needs a HIP device; there is no CPU path")
        self.device = torch.device("cuda")
        self.model_name = args.model_name
        self.converted_dir = os.path.join(args.save_dir, args.name, "converted_mel")
        os.makedirs(self.converted_dir, exist_ok=True)
        self.dataset_A, self.dataset_A_mean, self.dataset_A_std = load_speaker(args.preprocessed_data_dir, args.speaker_A_id)
        self.dataset_B, self.dataset_B_mean, self.dataset_B_std = load_speaker(args.preprocessed_data_dir, args.speaker_B_id)
        self.generator = Generator().to(self.device)
        self.generator.eval()
        self.saver = ModelSaver(args)
        self.saver.load_model(self.generator, self.model_name)
        self.vocoder = None
        if args.vocoder_ckpt:
            from .vocoder import MelVocoder
            self.vocoder = MelVocoder.from_checkpoint(args.vocoder_ckpt, self.device)
        elif getattr(args, "griffin_lim", 0) > 0:
            from .griffinlim import GriffinLimVocoder
            self.vocoder = GriffinLimVocoder(self.device, n_iter=args.griffin_lim, mel_inverse=getattr(args, "gl_mel_inverse", "pinv"),
                                             mel_iter=getattr(args, "gl_mel_iter", 64))
        if self.vocoder is not None:
            self.converted_audio_dir = os.path.join(args.save_dir, args.name, "converted_audio")
            os.makedirs(self.converted_audio_dir, exist_ok=True)
        self.out_rate = int(getattr(args, "out_sample_rate", None) or args.sample_rate)
        self.resampler = None
        if self.vocoder is not None and self.out_rate != int(args.sample_rate):
            from data_preprocessing.resample import Resampler
            from data_preprocessing.resample import ratio
            self.resampler = Resampler(self.device)
            self.resampler.table(*ratio(int(args.sample_rate), self.out_rate))      # uploaded once, before the two streams fork

    def wav_dir_utterances(self, mean, std):
        """--wav_dir: the folder's recordings (sorted) -> log-mels on the GPU (one launch) -> standardised with the SOURCE speaker's
        statistics, as the reference standardises what it feeds the generator (test.py:88-90)."""
        import glob
        from data_preprocessing.audio2mel import Audio2Mel, read_wav, read_wav_native
        files = sorted(glob.glob(os.path.join(self.args.wav_dir, "**", "*.wav"), recursive=True))
        if not files:
            raise ValueError("no .wav files under %s" % self.args.wav_dir)
        trim_db = getattr(self.args, "trim_silence", None)
        if trim_db is not None and getattr(self.args, "gpu_resample", False):
            native = [read_wav_native(f) for f in files]
            mels = Audio2Mel(self.device).bank_at_rates([x for _, x in native], [r for r, _ in native], trim_db=trim_db)
        elif trim_db is not None:
            mels = Audio2Mel(self.device).bank([read_wav(f) for f in files], trim_db=trim_db)
        elif getattr(self.args, "gpu_resample", False):
            native = [read_wav_native(f) for f in files]
            mels = Audio2Mel(self.device).bank_at_rates([x for _, x in native], [r for r, _ in native])
        else:
            mels = Audio2Mel(self.device).bank([read_wav(f) for f in files])
        return [((m - mean) / std).astype(np.float32) for m in mels]

    def write_audio(self, grp, converted, original, tag, st):
        """The reference's wav pair per utterance (test.py:94-103): both banks of equal-length mels are one batched decode each on the
        bucket's stream."""
        from scipy.io import wavfile
        with torch.cuda.stream(st):
            wavs = [self.vocoder.inverse(torch.from_numpy(np.stack(m)).to(self.device)) for m in (converted, original)]
            if self.resampler is not None:
                wavs = [self.resampler(w.reshape(w.shape[0], -1), int(self.args.sample_rate), self.out_rate) for w in wavs]
            wavs = [w.cpu().numpy() for w in wavs]
        for kind, wav in zip(("converted", "original"), wavs):
            for j, i in enumerate(grp):
                wavfile.write(os.path.join(self.converted_audio_dir, "%d-%s_%s.wav" % (i, kind, tag)), self.out_rate, wav[j])

    def test(self):
        a2b = self.model_name == "generator_A2B"
        src = self.dataset_A if a2b else self.dataset_B
        if self.args.wav_dir:
            src = self.wav_dir_utterances(*((self.dataset_A_mean, self.dataset_A_std) if a2b else (self.dataset_B_mean, self.dataset_B_std)))
        mean, std = (self.dataset_B_mean, self.dataset_B_std) if a2b else (self.dataset_A_mean, self.dataset_A_std)
        src_mean, src_std = (self.dataset_A_mean, self.dataset_A_std) if a2b else (self.dataset_B_mean, self.dataset_B_std)
        tag = ("%s_to_%s" % (self.args.speaker_A_id, self.args.speaker_B_id)) if a2b else ("%s_to_%s" % (self.args.speaker_B_id, self.args.speaker_A_id))
        outs = [None] * len(src)
        buckets = {}
        for i, mel in enumerate(src):
            buckets.setdefault(int(np.asarray(mel).shape[1]), []).append(i)
        self.generator.prepare_inference(self.args.dtype)      # weight packs are built once, on the current stream, before the lanes fork
        streams = [torch.cuda.Stream(device=self.device) for _ in range(2)]
        pending = []
        k = 0

        def drain(keep):
            """Write out the oldest groups until at most ``keep`` are in flight: device memory stays bounded by a few groups whatever the
            dataset size (the reference holds one utterance at a time, test.py:85-119)."""
            while len(pending) > keep:
                grp, fake, _real, ev, st = pending.pop(0)
                ev.synchronize()                              # the group's own stream is done with `fake` and `_real`
                host = fake.cpu().numpy()
                mels = [denormalize_mel(host[j], mean, std).astype(np.float32) for j in range(len(grp))]
                for j, i in enumerate(grp):
                    path = os.path.join(self.converted_dir, "%d-converted_%s.npy" % (i, tag))
                    np.save(path, mels[j])
                    outs[i] = path
                if self.vocoder is not None:
                    self.write_audio(grp, mels, [denormalize_mel(np.asarray(src[i], dtype=np.float32), src_mean, src_std).astype(np.float32) for i in grp],
                                     tag, st)
        with torch.no_grad():
            for T in sorted(buckets, reverse=True):
                ids = buckets[T]
                for lo in range(0, len(ids), max(1, self.args.max_batch)):
                    grp = ids[lo:lo + max(1, self.args.max_batch)]
                    st = streams[k % 2]; k += 1
                    st.wait_stream(torch.cuda.current_stream(self.device))
                    with torch.cuda.stream(st):
                        real = torch.from_numpy(np.stack([np.asarray(src[i], dtype=np.float32) for i in grp])).to(self.device, non_blocking=True)
                        fake = self.generator.infer(real, None, dtype=self.args.dtype).float()      # all-ones mask (test.py:92)
                        ev = torch.cuda.Event()
                        ev.record(st)
                    pending.append((grp, fake, real, ev, st))  # keep `real` alive until the stream is done with it
                    drain(4)                                  # two groups per stream in flight
            drain(0)
            for st in streams:
                torch.cuda.current_stream(self.device).wait_stream(st)
        print("wrote %d converted mel-spectrograms to %s" % (len(outs), self.converted_dir))
        return outs


def main(argv=None):
    args = CycleGANTestArgParser().parse_args(argv)
    MaskCycleGANVCTesting(args).test()


if __name__ == "__main__":
    main()
