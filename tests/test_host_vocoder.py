"""CPU: the host half of the MelGAN decoder -- weight-norm fold, state-dict key handling, sizes from the library, the new flag."""
import numpy as np
import pytest
import torch

import vocoder_checker as ck
from args.cycleGAN_test_arg_parser import CycleGANTestArgParser
from mask_cyclegan_vc import _hip
from mask_cyclegan_vc import vocoder as V


@pytest.mark.parametrize("mod", [torch.nn.Conv1d(6, 10, 3), torch.nn.ConvTranspose1d(6, 10, 4, stride=2, padding=1)], ids=["conv", "transposed"])
def test_weight_norm_fold_matches_torch(mod):
    torch.manual_seed(1)
    v = torch.randn_like(mod.weight, dtype=torch.float64)
    g = torch.rand(v.shape[0], 1, 1, dtype=torch.float64) + 0.5
    want = torch._weight_norm(v, g, 0)
    got = V.fold_weight_norm(g, v)
    assert got.dtype == torch.float64 and got.shape == mod.weight.shape
    assert float((got - want).abs().max()) <= 1e-12


def test_layer_table_is_the_published_state_dict():
    sd = ck.state_dict()
    assert len(sd) == 126
    names = [n for n, _ in V.layer_table()]
    assert len(names) == 42 and names[:5] == ["1", "3", "4.block.2", "4.block.4", "4.shortcut"] and names[-1] == "24"
    want = []
    for n, shape in V.layer_table():
        want += [("model.%s.bias" % n, (V.bias_len(n, shape),)), ("model.%s.weight_g" % n, (shape[0], 1, 1)), ("model.%s.weight_v" % n, shape)]
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want
    assert tuple(sd["model.3.weight_g"].shape) == (512, 1, 1) and tuple(sd["model.3.weight_v"].shape) == (512, 256, 16)


def test_state_dict_keys():
    sd = ck.state_dict()
    base = V.folded_layers(sd)
    assert len(base) == 42 and all(w.dtype == np.float32 and b.dtype == np.float32 for w, b in base)
    own = torch._weight_norm(sd["model.3.weight_v"], sd["model.3.weight_g"], 0).numpy()             # what the module itself multiplies with
    assert np.allclose(base[1][0], own, rtol=1e-6, atol=1e-9)

    def same(other):
        return all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(base, other))
    assert same(V.folded_layers({k[len("model."):]: v for k, v in sd.items()}))                     # no prefix
    assert same(V.folded_layers({"mel2wav." + k: v for k, v in sd.items()}))                        # the hub object's own prefix
    plain = {}
    for n, _shape in V.layer_table():                                                               # weight norm already removed
        plain["model.%s.weight" % n] = V.fold_weight_norm(sd["model.%s.weight_g" % n], sd["model.%s.weight_v" % n])
        plain["model.%s.bias" % n] = sd["model.%s.bias" % n]
    assert same(V.folded_layers(plain))
    missing = dict(sd)
    del missing["model.9.block.4.weight_g"]
    with pytest.raises(KeyError, match=r"model\.9\.block\.4\.weight_g"):
        V.folded_layers(missing)
    wrong = dict(sd)
    wrong["model.24.weight_v"] = torch.zeros(1, 32, 5)
    with pytest.raises(ValueError, match=r"model\.24\.weight_v"):
        V.folded_layers(wrong)
    extra = dict(sd)
    extra["model.26.bias"] = torch.zeros(1)
    with pytest.raises(ValueError, match=r"model\.26\.bias"):
        V.folded_layers(extra)


def test_sizes_from_the_library():
    L = _hip.lib()
    assert L.mcvc_voc_out_samples(4) == 1024 and L.mcvc_voc_out_samples(3) == 0 and L.mcvc_voc_out_samples(512) == 131072
    assert L.mcvc_voc_launches() == 30
    n_w = sum(int(np.prod(s)) + V.bias_len(n, s) for n, s in V.layer_table())
    assert n_w <= L.mcvc_voc_packed_floats() <= n_w + 4 * 42 + 2 * 256 * 16 * 512      # padding only; the stride-8 layers keep both groups' 2 taps
    assert L.mcvc_voc_workspace_floats(1, 3) == 0 and L.mcvc_voc_workspace_floats(0, 8) == 0
    prev = 0
    for B, T in [(1, 4), (1, 5), (2, 5), (2, 64), (3, 64), (16, 512)]:
        cur = L.mcvc_voc_workspace_floats(B, T)
        assert cur > prev and cur >= B * 32 * 256 * T
        prev = cur
    assert L.mcvc_voc_layer_packed_floats(V.KIND_CONV, 80, 512, 7, 1) >= 80 * 512 * 7 + 512
    assert L.mcvc_voc_layer_packed_floats(V.KIND_CONV, 80, 500, 7, 1) == 0               # rows must fill 32-row tiles
    assert L.mcvc_voc_layer_packed_floats(V.KIND_CONVT, 64, 32, 4, 3) == 0               # odd strides are not in this network


def test_packed_weights_hold_every_folded_weight():
    """mcvc_voc_pack moves values, it computes nothing but the sum of a block's two output biases: the packed buffer of the synthetic
    checkpoint holds exactly the multiset of folded weights."""
    import ctypes
    layers = V.folded_layers(ck.state_dict())
    L = _hip.lib()
    host = np.full(L.mcvc_voc_packed_floats(), np.nan, dtype=np.float32)
    table = (ctypes.c_void_p * 84)()
    for i, (w, b) in enumerate(layers):
        table[2 * i], table[2 * i + 1] = w.ctypes.data, b.ctypes.data
    assert L.mcvc_voc_pack(table, host.ctypes.data) == 0
    w0 = layers[0][0]
    n0 = w0.size
    assert np.array_equal(np.sort(host[:n0]), np.sort(w0.reshape(-1)))
    assert np.array_equal(host[n0:n0 + 512], layers[0][1])
    w_last, b_last = layers[-1]
    tail = host[-228:]
    assert np.array_equal(tail[:224], w_last.reshape(-1)) and tail[224] == b_last[0]
    table[5] = None
    assert L.mcvc_voc_pack(table, host.ctypes.data) == 1001


def test_vocoder_ckpt_flag():
    p = CycleGANTestArgParser().parser                       # (the bare parser: parse_args of the wrapper creates run directories)
    assert p.parse_args([]).vocoder_ckpt is None
    assert p.parse_args(["--vocoder_ckpt", "melgan.pt"]).vocoder_ckpt == "melgan.pt"
