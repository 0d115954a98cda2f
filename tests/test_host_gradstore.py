"""CPU-only: which parameter tensors a store pass covers (mcvc_grad_store_mask, include/mcvc.h MCVC_BWD_STORE_GRADS).

The mask is a static property of the layers (csrc/packforms.h grad_store_covered) that the fused update (zero_grads = 2 leaves exactly
these gradients uncleared) and the weight-gradient planner (exactly these are stored by a store pass) both read.  Here it is checked
against the networks' own parameter lists: the covered tensors are the weights of the Winograd layers (downSample1/2, upSample1/2), of the
1-D trunk (conv2dto1d, the residual blocks, conv1dto2d) and of the discriminators' three stride-2 layers -- never a bias, a norm affine
parameter, an edge layer (conv1, the last / output convolutions) or the unused downSample4 block -- and they hold more than 99 % of the
parameters (the share is printed: `GRADSTORE <net> covered <covered> of <all> = <share>`)."""
import ctypes

import pytest

from mask_cyclegan_vc import _hip
from mask_cyclegan_vc.model import Discriminator, Generator

MCVC_ERR_INVALID = 1001


def _mask(net, T=64):
    buf = (ctypes.c_ubyte * 128)(*([7] * 128))
    n = _hip.lib().mcvc_grad_store_mask(net, T, buf)
    return n, list(buf)


def _expected(net):
    mod = Generator() if net == 0 else Discriminator()
    names = [k for k, _ in mod.named_parameters()]
    want = []
    for k, p in mod.named_parameters():
        edge = p.dim() < 3 or p.shape[0] < 64 or p.shape[1] < 64 or "downSample4" in k          # vectors | 1 output / <= 2 input channels | dead block
        want.append(0 if edge else 1)
    return mod, names, want


@pytest.mark.parametrize("net", [0, 1])
def test_mask_covers_the_wide_weight_tensors_and_nothing_else(net):
    mod, names, want = _expected(net)
    n, got = _mask(net)
    assert n == len(names) == (110 if net == 0 else 20)
    assert got[n:] == [0] * (128 - n)                      # (all 128 bytes are written)
    numel = [p.numel() for p in mod.parameters()]
    if net == 1:                                           # the unused downSample4 block is neither updated nor covered
        numel = [0 if "downSample4" in k else m for k, m in zip(names, numel)]
    for k, g, w in zip(names, got[:n], want):
        assert g == w, (k, g, w)
    cov, tot = sum(m for m, g in zip(numel, got) if g), sum(numel)
    print("GRADSTORE %s covered %d of %d = %.5f" % ("generator" if net == 0 else "discriminator", cov, tot, cov / tot))
    assert cov / tot > 0.99


def test_mask_is_the_same_for_every_frame_count():
    for net in (0, 1):
        ref = _mask(net, 64)
        for T in (1, 40, 72, 128, 512):
            assert _mask(net, T) == ref


def test_bad_arguments_are_refused():
    L = _hip.lib()
    buf = (ctypes.c_ubyte * 128)()
    assert L.mcvc_grad_store_mask(2, 64, buf) == MCVC_ERR_INVALID
    assert L.mcvc_grad_store_mask(-1, 64, buf) == MCVC_ERR_INVALID
    assert L.mcvc_grad_store_mask(0, 0, buf) == MCVC_ERR_INVALID
    assert L.mcvc_grad_store_mask(0, 64, None) == MCVC_ERR_INVALID
