"""The MelGAN vocoder object the reference holds (``torch.hub.load('descriptinc/melgan-neurips', 'load_melgan')``: test.py:46-47,
utils.py:25-39, preprocess_vcc2018.py:26-60), restated from its published definition and run on the HIP kernels:

* ``vocoder(audio)``    waveform -> log-mel, ``data_preprocessing.audio2mel.Audio2Mel`` (csrc/audio_kernels.hip);
* ``vocoder.inverse(mel)``  log-mel [B, 80, T] -> waveform [B, 256 T], the MelGAN generator of Kumar et al. 2019,
  ``Generator(input_size=80, ngf=32, n_residual_layers=3)`` (csrc/vocoder_kernels.hip through ``mcvc_voc_decode``): fp32, inference
  only, 30 launches per call for the whole batch.  There is no CPU path.

Weights.  No trained MelGAN weights ship with this project and none can be fetched here; ``load_state_dict`` takes the hub checkpoint's
state dict (126 tensors: 42 layers x ``bias``, ``weight_g``, ``weight_v``, names ``model.<i>...`` or ``mel2wav.model.<i>...``-style
prefixes stripped down to the module index) or the same layers with plain ``weight`` keys.  Weight norm is folded once, in float64:
``w = g * v / ||v||`` with the norm over every dimension but 0 (for a transposed convolution that is per INPUT channel).
"""
import ctypes

import numpy as np
import torch

from . import _hip

N_MEL = 80
HOP = 256
MIN_FRAMES = 4
STAGES = ((8, 512, 256), (8, 256, 128), (2, 128, 64), (2, 64, 32))          # (stride r, Cin, Cout): ConvTranspose1d(Cin, Cout, 2r, r)


def layer_table():
    """The 42 Conv1d / ConvTranspose1d modules in state-dict order: (name, weight shape in torch's layout)."""
    out = [("1", (512, N_MEL, 7))]
    i = 2
    for r, cin, cout in STAGES:
        out.append((str(i + 1), (cin, cout, 2 * r)))                         # i: LeakyReLU, i + 1: the transposed conv
        for j in range(3):
            blk = str(i + 2 + j)
            out += [(blk + ".block.2", (cout, cout, 3)), (blk + ".block.4", (cout, cout, 1)), (blk + ".shortcut", (cout, cout, 1))]
        i += 5
    out.append((str(i + 2), (1, 32, 7)))                                     # i: LeakyReLU, i + 1: ReflectionPad1d, i + 2: the last conv
    return out


def bias_len(name, shape):
    """A Conv1d's bias has shape[0] entries, a ConvTranspose1d's ([Cin][Cout][k]) shape[1]."""
    return shape[1] if _is_transposed(name) else shape[0]


def _is_transposed(name):
    return name in ("3", "8", "13", "18")


def fold_weight_norm(g, v):
    """w = g * v / ||v||, the norm over every dimension but 0 (torch.nn.utils.weight_norm, dim=0), in float64."""
    g = torch.as_tensor(g).detach().to("cpu", torch.float64)
    v = torch.as_tensor(v).detach().to("cpu", torch.float64)
    n = v.reshape(v.shape[0], -1).norm(dim=1).reshape([-1] + [1] * (v.dim() - 1))
    return g.reshape(n.shape) * v / n


def _strip(key):
    """'model.4.block.2.weight_v', 'mel2wav.model.4...', '4.block.2.weight_v' -> '4.block.2.weight_v'."""
    parts = key.split(".")
    if "model" in parts:
        parts = parts[parts.index("model") + 1:]
    return ".".join(parts)


def folded_layers(state_dict):
    """state dict -> list of 42 (weight, bias) float32 numpy pairs in ``layer_table`` order.  Raises KeyError naming a missing key,
    ValueError naming a key of the wrong shape or one that belongs to no layer."""
    sd = {}
    for k, v in state_dict.items():
        s = _strip(k)
        if s in sd:
            raise ValueError("state dict holds %r twice (as %r)" % (s, k))
        sd[s] = v
    used, out = set(), []

    def take(key, shape):
        if key not in sd:
            raise KeyError("MelGAN state dict: missing key model.%s" % key)
        t = torch.as_tensor(sd[key]).detach().cpu()
        if tuple(t.shape) != tuple(shape):
            raise ValueError("MelGAN state dict: model.%s has shape %s, expected %s" % (key, tuple(t.shape), tuple(shape)))
        used.add(key)
        return t

    for name, shape in layer_table():
        if name + ".weight" in sd:
            w = take(name + ".weight", shape).to(torch.float64)
        else:
            g = take(name + ".weight_g", (shape[0], 1, 1))
            v = take(name + ".weight_v", shape)
            w = fold_weight_norm(g, v)
        b = take(name + ".bias", (bias_len(name, shape),))
        out.append((np.ascontiguousarray(w.numpy(), dtype=np.float32), np.ascontiguousarray(b.to(torch.float64).numpy(), dtype=np.float32)))
    extra = sorted(set(sd) - used)
    if extra:
        raise ValueError("MelGAN state dict: unexpected key model.%s" % extra[0])
    return out


class MelVocoder(object):
    """``MelVocoder().load_state_dict(sd)`` / ``MelVocoder.from_checkpoint(path)``; then ``inverse(mel)`` and ``__call__(audio)``."""

    def __init__(self, device=None):
        self.device = _hip.hip_device("mask_cyclegan_vc.vocoder", device)
        self.packed = None
        self._fft = None

    @classmethod
    def from_checkpoint(cls, path, device=None):
        sd = torch.load(path, map_location="cpu")
        voc = cls(device)
        voc.load_state_dict(sd)
        return voc

    def load_state_dict(self, state_dict):
        layers = folded_layers(state_dict)
        L = _hip.lib()
        host = np.zeros(L.mcvc_voc_packed_floats(), dtype=np.float32)
        table = (ctypes.c_void_p * (2 * len(layers)))()
        for i, (w, b) in enumerate(layers):
            table[2 * i], table[2 * i + 1] = w.ctypes.data, b.ctypes.data
        _hip.check(L.mcvc_voc_pack(table, host.ctypes.data), "mcvc_voc_pack")
        self.packed = torch.from_numpy(host).to(self.device)
        return self

    def inverse(self, mel):
        """[B, 80, T] log10-mel on the HIP device -> [B, 256 T] float32 waveform; one batched decode on the current stream."""
        if self.packed is None:
            raise RuntimeError("MelVocoder: no weights loaded (load_state_dict / from_checkpoint)")
        _hip.require_on_device("mask_cyclegan_vc.vocoder", mel, self.device, "mel", "vocoder")
        if mel.dim() != 3 or mel.shape[1] != N_MEL:
            raise ValueError("expected a [B, 80, T] mel tensor, got %s" % (tuple(mel.shape),))
        B, _, T = mel.shape
        if T < MIN_FRAMES:
            raise ValueError("the MelGAN decoder needs at least %d frames (ReflectionPad1d(3)), got %d" % (MIN_FRAMES, T))
        if B < 1:
            raise ValueError("empty batch")
        L = _hip.lib()
        with torch.no_grad(), torch.cuda.device(self.device):
            x = mel.detach().to(torch.float32).contiguous()
            n = L.mcvc_voc_workspace_floats(B, T)
            ws = torch.empty(n, dtype=torch.float32, device=self.device)
            out = torch.empty(B, L.mcvc_voc_out_samples(T), dtype=torch.float32, device=self.device)
            _hip.check(L.mcvc_voc_decode(_hip.ptr(self.packed), _hip.ptr(x), _hip.ptr(out), _hip.ptr(ws), n, B, T, _hip.stream()), "mcvc_voc_decode")
        return out

    def __call__(self, audio):
        from data_preprocessing.audio2mel import Audio2Mel
        if self._fft is None:
            self._fft = Audio2Mel(self.device)
        return self._fft(audio)


KIND_CONV, KIND_CONVT, KIND_STACK, KIND_LAST = 0, 1, 2, 3


def run_layer(kind, x0, w0, b0, x1=None, w1=None, b1=None, dilation=1, r=1, act_in=False, out=None):
    """ONE layer of the decoder through the kernels ``inverse`` runs (``mcvc_voc_layer``; op-level parity tests).  ``w*`` / ``b*`` are
    folded weights in torch's layouts (any device; packed on the host), ``x*`` HIP-device tensors [B, C, L].  ``out``: a 16-byte aligned
    contiguous destination of the result's size, else a new tensor.  kind: KIND_CONV (reflection padding), KIND_CONVT (k = 2r, stride r),
    KIND_STACK (w0 @ x0 + b0 + w1 @ lrelu(x1) + b1), KIND_LAST (LeakyReLU + conv to one channel + tanh)."""
    _hip.require_cuda_f32(x0, x1)
    L = _hip.lib()
    f = lambda t: None if t is None else np.ascontiguousarray(torch.as_tensor(t).detach().cpu().numpy(), dtype=np.float32)
    p = lambda a: None if a is None else a.ctypes.data
    w0, b0, w1, b1 = f(w0), f(b0), f(w1), f(b1)
    B, Cin, n = x0.shape
    Cout, k = (w0.shape[1], w0.shape[2]) if kind == KIND_CONVT else (w0.shape[0], w0.shape[2])
    floats = L.mcvc_voc_layer_packed_floats(kind, Cin, Cout, k, r)
    if floats == 0:
        raise ValueError("not a layer shape the decoder kernels take")
    host = np.zeros(floats, dtype=np.float32)
    _hip.check(L.mcvc_voc_layer_pack(kind, p(w0), p(b0), p(w1), p(b1), host.ctypes.data, Cin, Cout, k, r), "mcvc_voc_layer_pack")
    packed = torch.from_numpy(host).to(x0.device)
    shape = (B, n) if kind == KIND_LAST else (B, Cout, n * (r if kind == KIND_CONVT else 1))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x0.device)
    if out.numel() != int(np.prod(shape)) or not out.is_contiguous():
        raise ValueError("destination of the wrong size")
    _hip.check(L.mcvc_voc_layer(kind, _hip.ptr(packed), _hip.ptr(x0), _hip.ptr(x1), _hip.ptr(out), B, Cin, Cout, n, k, dilation, r, int(bool(act_in)),
                                _hip.stream()), "mcvc_voc_layer")
    return out.view(shape)
