"""The restricted re-packs and fused updates write exactly the regions their plan lists (mcvc_pack_plan, tests/test_host_packplan.py), and a
pass that would read a form the last re-pack of its buffer did not refresh is refused instead of reading old weights.

Shapes: T = 32 is the smallest frame count of the Winograd-only tables, T = 64 the smallest at which upSample2 drops its 36-point sets;
max_batch 1 and 4 select the small-batch and the F(4x4,3x3) schedules."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import mcvc_oracle as orc  # noqa: E402
from mask_cyclegan_vc.model import Discriminator, Generator  # noqa: E402
from test_hip_update import _flat_group  # noqa: E402
from test_host_packplan import plan  # noqa: E402

MCVC_ERR_INVALID = 1001
SENTINEL = 0x7FC0DEAD          # a NaN pattern no pack kernel produces; buffers are compared as integers


def _sentinel(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _mark(mask, rows):
    for dst, ln in {(int(r[5]), int(r[6])) for r in rows[rows[:, 0] == 1]}:
        mask[dst:dst + ln] = True
    return mask


def _check_regions(buf, full, mask, what):
    b, f = buf.view(torch.int32), full.view(torch.int32)
    torch.cuda.synchronize()
    assert bool(mask.any()), what
    assert bool(((b == f) | ~mask).all()), (what, "a listed region differs from the full pack", int(((b != f) & mask).sum()))
    assert bool(((b == SENTINEL) | mask).all()), (what, "written outside the listed regions", int(((b != SENTINEL) & ~mask).sum()))


class _Net:
    """A network in the engine's flat layout with zero gradients and moments: an update with lr = 0 leaves the parameters as they are."""

    def __init__(self, mod, seed_key, seed, live=None):
        from mask_cyclegan_vc._hip import ptr_table
        mod.load_state_dict(orc.filler_params(seed_key, seed), strict=True)
        self.ps, self.flat, offs = _flat_group(mod.cuda(), live)
        self.tab = ptr_table(self.ps)
        live = set(range(len(self.ps))) if live is None else set(live)
        self.numel = (ctypes.c_longlong * len(self.ps))(*[p.numel() if i in live else 0 for i, p in enumerate(self.ps)])
        self.zeros = [torch.zeros_like(self.flat) for _ in range(3)]

    def opt(self):
        from mask_cyclegan_vc._hip import ptr, stream
        g, m, v = self.zeros
        return (ptr(self.flat), ptr(g), None, ptr(m), ptr(v), 0.0, 0.5, 0.999, 1e-8, 1, 1.0, 0, stream())


@pytest.fixture(scope="module")
def gen():
    from mask_cyclegan_vc._hip import check, lib, ptr, stream
    net = _Net(Generator(), "G", 23)
    net.full = _sentinel(lib().mcvc_gen_packed_floats())
    check(lib().mcvc_gen_pack(net.tab, ptr(net.full), stream()), "pack")
    return net


@pytest.mark.parametrize("max_batch,T", [(1, 32), (4, 32), (1, 64), (4, 64)])
def test_generator_entries_write_exactly_their_planned_regions(gen, max_batch, T):
    from mask_cyclegan_vc._hip import check, lib, ptr, stream
    L = lib()
    n = gen.full.numel()
    new_mask = lambda: torch.zeros(n, dtype=torch.bool, device="cuda")
    buf = _sentinel(n)
    check(L.mcvc_gen_pack_sets(gen.tab, ptr(buf), max_batch, T, 1, stream()), "sets 1")
    mask = _mark(new_mask(), plan(0, max_batch, T, 1, 7, 0))
    _check_regions(buf, gen.full, mask, "sets=1")
    check(L.mcvc_gen_pack_sets(gen.tab, ptr(buf), max_batch, T, 2, stream()), "sets 2")
    _check_regions(buf, gen.full, _mark(mask, plan(0, max_batch, T, 2, 7, 0)), "sets=1 then 2")
    both = _mark(new_mask(), plan(0, max_batch, T, 3, 7, 0))
    assert torch.equal(mask, both)                   # the two halves are the whole re-pack
    for r in (1, 2, 8, 16, 32, 4):
        buf = _sentinel(n)
        check(L.mcvc_gen_pack_ranges(gen.tab, ptr(buf), max_batch, T, 3, r, stream()), "ranges")
        _check_regions(buf, gen.full, _mark(new_mask(), plan(0, max_batch, T, 3, r, 0)), "range %d" % r)
    for r in (7, 1, 2, 8, 16, 32, 4):
        buf = _sentinel(n)
        keep = gen.flat.clone()
        check(L.mcvc_gen_update_ranges(gen.tab, gen.numel, ptr(buf), max_batch, T, r, *gen.opt()), "update")
        _check_regions(buf, gen.full, _mark(new_mask(), plan(0, max_batch, T, 3, r, 1)), "update range %d" % r)
        assert torch.equal(keep, gen.flat)


@pytest.mark.parametrize("max_batch,T", [(1, 64), (4, 64), (2, 68)])
def test_discriminator_entries_write_exactly_their_planned_regions(max_batch, T):
    from mask_cyclegan_vc._hip import check, lib, ptr, stream
    L = lib()
    live = [i for i in range(20) if not 14 <= i < 18]           # (downSample4 is dead: neither updated nor packed)
    net = _Net(Discriminator(), "D", 29, live)
    n = L.mcvc_disc_packed_floats()
    full = _sentinel(n)
    check(L.mcvc_disc_pack(net.tab, ptr(full), stream()), "pack")
    for update in (0, 1):
        buf = _sentinel(n)
        if update:
            check(L.mcvc_disc_update_batch(net.tab, net.numel, ptr(buf), max_batch, T, *net.opt()), "update")
        else:
            check(L.mcvc_disc_pack_batch(net.tab, ptr(buf), max_batch, T, stream()), "pack_batch")
        mask = _mark(torch.zeros(n, dtype=torch.bool, device="cuda"), plan(1, max_batch, T, 3, 7, update))
        _check_regions(buf, full, mask, "disc update=%d" % update)


def _gen_pass(gen, packed, B, T, x, dout):
    from mask_cyclegan_vc._hip import lib, ptr, ptr_table, stream
    L = lib()
    n_scr = L.mcvc_gen_scratch_floats(B, T)
    stash = torch.zeros(L.mcvc_gen_stash_floats(B, T), device="cuda"); scr = torch.zeros(n_scr, device="cuda")
    out = torch.empty(B, 80, L.mcvc_gen_out_frames(T), device="cuda")
    grads = [torch.zeros_like(p) for p in gen.ps]
    m = torch.ones_like(x)
    rc_f = L.mcvc_gen_forward(gen.tab, ptr(packed), ptr(x), ptr(m), ptr(out), ptr(stash), ptr(scr), n_scr, B, T, stream())
    rc_b = None
    if rc_f == 0:
        rc_b = L.mcvc_gen_backward(gen.tab, ptr(packed), ptr_table(grads), ptr(m), ptr(dout), None, 0, ptr(stash), ptr(scr), n_scr, B, T, stream(), None)
    torch.cuda.synchronize()
    return rc_f, rc_b, out, grads


def test_backward_is_refused_until_the_backward_forms_are_fresh(gen):
    """(tests/test_hip_model.py has the T = 64 case; here the Winograd-only table of T = 32 at max_batch 4.)"""
    from mask_cyclegan_vc._hip import check, lib, ptr, stream
    L = lib()
    B, T, max_batch = 1, 32, 4
    x = torch.randn(B, 80, T, device="cuda"); dout = torch.randn(B, 80, T, device="cuda")
    L.mcvc_set_deterministic(1)
    try:
        full = torch.zeros_like(gen.full)
        check(L.mcvc_gen_pack(gen.tab, ptr(full), stream()), "pack")
        rc_f, rc_b, out_ref, grads_ref = _gen_pass(gen, full, B, T, x, dout)
        assert rc_f == 0 and rc_b == 0
        two = torch.zeros_like(gen.full)
        check(L.mcvc_gen_pack_sets(gen.tab, ptr(two), max_batch, T, 1, stream()), "sets 1")
        rc_f, rc_b, out, grads = _gen_pass(gen, two, B, T, x, dout)
        assert rc_f == 0 and rc_b == MCVC_ERR_INVALID and torch.equal(out, out_ref)
        assert all(float(g.abs().max()) == 0.0 for g in grads)            # refused before anything ran
        check(L.mcvc_gen_pack_sets(gen.tab, ptr(two), max_batch, T, 2, stream()), "sets 2")
        rc_f, rc_b, out, grads = _gen_pass(gen, two, B, T, x, dout)
        assert rc_f == 0 and rc_b == 0 and torch.equal(out, out_ref)
        assert all(torch.equal(a, b) for a, b in zip(grads, grads_ref))
    finally:
        L.mcvc_set_deterministic(0)


def test_pass_at_another_frame_count_reads_no_stale_set(gen):
    """The T = 64 table of one sample per pass drops upSample2's 36-point sets (every pass there takes F(4x4,5x5)).  A pass at T = 40 on
    the same buffer -- 20 x 10 and 40 x 20 images, too few tiles for F(4x4) -- would need them: refused.  After a full pack it runs."""
    from mask_cyclegan_vc._hip import check, lib, ptr, stream
    L = lib()
    packed = torch.zeros_like(gen.full)
    check(L.mcvc_gen_pack_sets(gen.tab, ptr(packed), 1, 64, 3, stream()), "pack T=64")
    x64 = torch.randn(1, 80, 64, device="cuda"); x40 = torch.randn(1, 80, 40, device="cuda")
    assert _gen_pass(gen, packed, 1, 64, x64, x64)[:2] == (0, 0)
    assert _gen_pass(gen, packed, 1, 40, x40, x40)[0] == MCVC_ERR_INVALID
    check(L.mcvc_gen_pack(gen.tab, ptr(packed), stream()), "pack")
    assert _gen_pass(gen, packed, 1, 40, x40, x40)[:2] == (0, 0)


def test_layer_shapes_that_collided_in_the_old_table_key_get_their_own_tables():
    """The op-level pack used to cache its job table under a hash of the layer shape; (Cin, Cout) = (8, 39) and (9, 8) hashed alike
    (8 * 31 + 39 == 9 * 31 + 8), so the second would have been packed with the first one's jobs.  The key is the shape itself now.
    Bound: a K = 81 fp32 dot product carries at most K * 2^-24 ~ 5e-6 relative rounding (asserted with a factor 4); a wrongly packed layer is off by O(1)."""
    from mask_cyclegan_vc._hip import check, lib, ptr, stream
    L = lib()
    N, H, W = 1, 8, 8
    g = torch.Generator().manual_seed(3)
    for Cin, Cout in ((8, 39), (9, 8)):
        spec = (Cin, Cout, 1, 3, 3, 1, 1, 1)
        w = torch.randn(Cout, Cin, 3, 3, generator=g); b = torch.randn(Cout, generator=g); x = torch.randn(N, Cin, H, W, generator=g)
        ref = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), padding=1)
        wd, bd, xd = w.cuda(), b.cuda(), x.cuda()
        packed = torch.zeros(L.mcvc_layer_packed_floats(*spec), device="cuda")
        check(L.mcvc_layer_pack(ptr(wd), ptr(bd), None, None, ptr(packed), *spec, stream()), "layer_pack")
        n_scr = L.mcvc_layer_scratch_floats(N, H, W, *spec)
        scratch = torch.zeros(n_scr, device="cuda"); y = torch.zeros(N, Cout, H, W, device="cuda")
        check(L.mcvc_layer_forward(ptr(xd), ptr(packed), ptr(wd), None, ptr(y), ptr(scratch), n_scr, N, H, W, *spec, 4, 0, stream()), "layer_forward")
        torch.cuda.synchronize()
        err = float((y.cpu().double() - ref).norm() / ref.norm())
        print("Cin=%d Cout=%d rel-L2 %.3e" % (Cin, Cout, err))
        assert err < 2e-5, (Cin, Cout, err)
