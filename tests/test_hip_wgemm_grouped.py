"""GPU: the weight gradients' K split in a grouped discriminator pass (csrc/net.hip conv_wgrad, the implicit wgemm path).

The split of the implicit weight gradient is planned per network (128 workgroups), so that a grouped launch (both networks in one grid,
csrc/twin.h) stays within one round on the chip.  A grouped pass and the single passes must plan the same split: a grouped
discriminator forward + backward must equal the two single passes bit for bit, at batches whose weight gradients split (1, 2) and at
one that runs several rounds (8)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import mcvc_oracle as orc  # noqa: E402  (parameter filler only)
from mask_cyclegan_vc import _hip  # noqa: E402
from mask_cyclegan_vc._hip import check, lib, ptr, ptr_table, stream  # noqa: E402
from mask_cyclegan_vc.model import Discriminator  # noqa: E402

T = 64


@pytest.fixture
def deterministic_mode():
    L = lib()
    was = L.mcvc_set_deterministic(1)
    yield
    L.mcvc_set_deterministic(was)


def _pass(L, d, x, dout, B):
    """One discriminator forward + backward on the C ABI: returns (out, dx, flat weight gradients, packed, params) and the closure that runs it."""
    params = list(d.parameters())
    packed = d.packed_weights(params)
    stash = torch.zeros(L.mcvc_disc_stash_floats(B, T), device="cuda")
    scratch = torch.zeros(L.mcvc_disc_scratch_floats(B, T), device="cuda")
    out = torch.zeros((B, 1, 10, L.mcvc_disc_out_frames(T)), device="cuda")
    sizes = [0 if 14 <= i <= 17 else p.numel() for i, p in enumerate(params)]      # (downSample4 takes no part in forward)
    flat = torch.zeros(sum((n + 3) & ~3 for n in sizes), device="cuda")
    grads, off = [], 0
    for p, n in zip(params, sizes):
        grads.append(flat[off:off + n].view_as(p) if n else None)
        off += (n + 3) & ~3
    dx = torch.zeros((B, 80, T), device="cuda")
    ptab, gtab = ptr_table(params), ptr_table(grads)

    def run():
        check(L.mcvc_disc_forward(ptab, ptr(packed), ptr(x), ptr(out), ptr(stash), ptr(scratch), scratch.numel(), B, T, stream()),
              "mcvc_disc_forward")
        check(L.mcvc_disc_backward(ptab, ptr(packed), gtab, ptr(dout), 0, ptr(dx), 0, ptr(stash), ptr(scratch), scratch.numel(), B, T,
                                   stream(), None), "mcvc_disc_backward")
    return (out, dx, flat, packed, params), run


@pytest.mark.parametrize("B", [1, 2, 8])
def test_grouped_discriminator_backward_equals_the_single_passes(deterministic_mode, B):
    L = lib()
    nets = []
    for i in range(2):
        d = Discriminator()
        d.load_state_dict(orc.filler_params("D", 820 + i), strict=True)
        nets.append(d.cuda())
    g = torch.Generator().manual_seed(B)
    xs = [torch.randn(B, 80, T, generator=g).cuda() for _ in range(2)]
    douts = [torch.randn(B, 1, 10, L.mcvc_disc_out_frames(T), generator=g).cuda() for _ in range(2)]

    single = []
    for i in range(2):
        res, run = _pass(L, nets[i], xs[i], douts[i], B)
        run()
        single.append(res)
    torch.cuda.synchronize()

    twin = [_pass(L, nets[i], xs[i], douts[i], B) for i in range(2)]
    with _hip.twin() as tw:
        twin[0][1]()
        tw.switch()
        twin[1][1]()
    torch.cuda.synchronize()
    for i in range(2):
        out_s, dx_s, g_s = single[i][:3]
        out_t, dx_t, g_t = twin[i][0][:3]
        assert torch.equal(out_s, out_t), i
        assert torch.equal(dx_s, dx_t), i
        assert torch.equal(g_s, g_t), i
        assert float(dx_s.abs().max()) > 0.0 and float(g_s.abs().max()) > 0.0
    assert not torch.equal(single[0][1], single[1][1])

