"""Time and effect of the mel inversion (csrc/melinv_kernels.hip, mask_cyclegan_vc.melinv.MelInverter).  Informational, not a gate.

Time: a VCC2018-like set of 35 utterances of 150 .. 900 frames (the set of tools/f0_bench.py and tools/ms_bench.py), HIP events around
many calls after a warm-up, through the C ABI on buffers made once: one solve per utterance (what the inference driver does, a launch
each), the same frames as ONE call on the concatenation (a frame does not depend on T), the start value alone (n_iter = 0), and beside
them one Griffin-Lim decode of the same set (32 iterations, one decode per utterance).

Effect, on the two committed recordings, for the clamped pseudo-inverse and for the solver at --mel_iter, with the Griffin-Lim loop at
32 iterations from the seeded angles: || M - S || / || S || of the magnitude M that goes into the loop against the front-end's true
magnitude S (float64 STFT of the recording), the same for |STFT(decoded audio)|, and the RMS difference in dB between the front-end's
log-mel of the decoded audio and the input log-mel.

    python tools/melinv_bench.py [--iters 20] [--warmup 5] [--utts 35] [--mel_iter 64] [--gl_iter 32] [--timing_only] [--out profiles/melinv_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "maskcyclegan-vc_amd"), os.path.join(ROOT, "tests")]

import griffinlim_checker as glck  # noqa: E402
import melinv_checker as ck  # noqa: E402
from data_preprocessing.audio2mel import Audio2Mel, read_wav  # noqa: E402
from mask_cyclegan_vc import _hip  # noqa: E402
from mask_cyclegan_vc.griffinlim import GriffinLimVocoder  # noqa: E402
from mask_cyclegan_vc.melinv import MelInverter  # noqa: E402


def timed(fn, warmup, iters, inner=1):
    """-> (median, min, max) ms per call of ``fn``; ``inner`` calls between one pair of events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    ms.sort()
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--utts", type=int, default=35)
    ap.add_argument("--mel_iter", type=int, default=64)
    ap.add_argument("--gl_iter", type=int, default=32)
    ap.add_argument("--timing_only", action="store_true")
    ap.add_argument("--out", type=str, default=None, help="also write the figures to this JSON file")
    a = ap.parse_args()
    L = _hip.lib()
    inv, gl = MelInverter(n_iter=a.mel_iter), GriffinLimVocoder(n_iter=a.gl_iter)
    rs = np.random.RandomState(0)
    frames = rs.randint(150, 901, size=a.utts)
    total = int(frames.sum())
    mels = [torch.from_numpy((-2.0 + np.cumsum(0.05 * rs.randn(1, 80, T), axis=2) + 0.1 * rs.randn(1, 80, T)).astype(np.float32)).cuda() for T in frames]
    res = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(_hip.LIB_PATH), "tile_frames": int(os.environ.get("MCVC_MELINV_TF", "16")),
           "utterances": a.utts, "frames_min": int(frames.min()), "frames_max": int(frames.max()), "frames_total": total, "mel_iter": a.mel_iter,
           "gl_iter": a.gl_iter, "iters": a.iters, "warmup": a.warmup}
    print("%d utterances, %d .. %d frames, %d frames in all; solver steps %d, Griffin-Lim iterations %d" % (a.utts, frames.min(), frames.max(), total, a.mel_iter, a.gl_iter))

    tables = inv.tables()
    outs = [torch.empty(1, 513, int(T), dtype=torch.float32, device="cuda") for T in frames]
    cat = torch.cat(mels, dim=2).contiguous()
    cat_out = torch.empty(1, 513, total, dtype=torch.float32, device="cuda")

    def per_utterance(n):
        def fn():
            for m, o in zip(mels, outs):
                _hip.check(L.mcvc_melinv_solve(_hip.ptr(m), _hip.ptr(tables), _hip.ptr(o), 1, m.shape[2], n, _hip.stream()), "mcvc_melinv_solve")
        return fn

    def one_call(n):
        return lambda: _hip.check(L.mcvc_melinv_solve(_hip.ptr(cat), _hip.ptr(tables), _hip.ptr(cat_out), 1, total, n, _hip.stream()), "mcvc_melinv_solve")

    for key, fn in (("solve_per_utterance_ms", per_utterance(a.mel_iter)), ("solve_one_call_ms", one_call(a.mel_iter)),
                    ("start_value_per_utterance_ms", per_utterance(0)), ("start_value_one_call_ms", one_call(0))):
        res[key] = timed(fn, a.warmup, a.iters, inner=10)
        print("%-30s median %.4f ms for the set (min %.4f max %.4f), 10 sets per window" % (key, res[key]["median"], res[key]["min"], res[key]["max"]))
    per_utterance(a.mel_iter)()
    one_call(a.mel_iter)()
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(outs, dim=2), cat_out), "one call on the concatenation is not the per-utterance result"
    res["us_per_frame_and_step"] = 1e3 * (res["solve_one_call_ms"]["median"] - res["start_value_one_call_ms"]["median"]) / total / max(a.mel_iter, 1)

    if not a.timing_only:
        angles = [gl.angles(1, int(T)) for T in frames]

        def decode():
            for m, ang in zip(mels, angles):
                gl.inverse(m, angles=ang)
        res["griffin_lim_decode_per_utterance_ms"] = timed(decode, 1, 3)
        g = res["griffin_lim_decode_per_utterance_ms"]
        print("Griffin-Lim decode of the set, %d iterations: median %.2f ms (min %.2f max %.2f) -- the solver adds %.2f %% to it"
              % (a.gl_iter, g["median"], g["min"], g["max"], 100.0 * res["solve_per_utterance_ms"]["median"] / g["median"]))
        res["solver_over_decode"] = res["solve_per_utterance_ms"]["median"] / g["median"]

        fft = Audio2Mel()
        glN = GriffinLimVocoder(n_iter=a.gl_iter, mel_inverse="nnls", mel_iter=a.mel_iter)
        res["clips"] = {}
        for name in ("real_VCC2SF3.wav", "real_VCC2TF1.wav"):
            x = read_wav(os.path.join(ROOT, "tests", "golden", "audio", name))
            (mel,) = fft.bank([x])
            S = glck.stft(x.astype(np.float64)[None]).abs().numpy()
            T = mel.shape[1]
            assert S.shape[2] == T
            md = torch.from_numpy(mel[None]).cuda()
            row = {"frames": int(T)}
            for how, dec, M in (("pinv", gl, inv(md, n_iter=0)), ("nnls", glN, inv(md))):
                wav = dec.inverse(md)[0].cpu().numpy()
                (again,) = fft.bank([wav])
                Sd = glck.stft(wav.astype(np.float64)[None]).abs().numpy()
                Mh = M.cpu().numpy()
                row[how] = {"mel_residual": ck.mel_residual(Mh, mel[None]), "M_vs_S": ck.relative_distance(Mh, S),
                            "decoded_stft_vs_S": ck.relative_distance(Sd, S), "decoded_stft_vs_M": ck.relative_distance(Sd, Mh),
                            "decoded_logmel_rms_db": float(20.0 * np.sqrt(np.mean((again.astype(np.float64) - mel) ** 2)))}
                print("%s %s: ||B M - y|| / ||y|| %.3e   ||M - S|| / ||S|| %.4f   after the loop: || |STFT(wav)| - S || / ||S|| %.4f, against M %.4f, "
                      "log-mel of the decoded audio against the input %.3f dB RMS" % (name, how, row[how]["mel_residual"], row[how]["M_vs_S"],
                                                                                      row[how]["decoded_stft_vs_S"], row[how]["decoded_stft_vs_M"], row[how]["decoded_logmel_rms_db"]))
            res["clips"][name] = row
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
