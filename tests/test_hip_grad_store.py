"""GPU: gradient store mode (include/mcvc.h MCVC_BWD_STORE_GRADS, zero_grads = 2, engine.grad_store).

A fused update with zero_grads = 2 leaves the gradients of the covered tensors (mcvc_grad_store_mask: > 99 % of the parameters) as they
are and clears only the rest; the first weight-gradient pass of the next iteration STORES the covered gradients instead of adding to
zeros.  What must hold, and is checked here on the C ABI and on the engine:

  1. one store pass over a buffer whose covered tensors hold NaN leaves exactly what a plain pass leaves in an all-zero buffer -- for every
     writer the planner picks (persistent / per-layer trunk, F(4x4) / F(2x2) Winograd, un-split wgemm next to split dw_accum, a Winograd
     pass in several sample chunks) and for the writers that can only add, in front of which the tensor is zero-filled (T = 72);
  2. a plain pass behind a store pass still accumulates;
  3. the same with floating-point atomics on (default mode), to rounding;
  4. update mode 2 computes what mode 1 computes and leaves exactly the masked gradients alone;
  5. five engine steps with grad_store on and off are equal, whatever the schedule, and never read a stale covered gradient -- neither
     where the first pass stores (the grouped / pipelined schedules, the split discriminator halves at B = 8 included) nor where a path
     that can only add meets a store-ready buffer and must zero it (a larger batch on the four-lane schedule, a schedule change, a phase
     called on its own).

"Equal" is `==` on every element in deterministic mode (mcvc_set_deterministic(1)): -0.0 and +0.0 agree (a stored -0.0 is a sum's +0.0),
a NaN never passes.  The default-mode gate is 5e-5 relative L2 per tensor, the figure tests/test_hip_ops_modes.py applies to a layer's
weight gradients in either mode.

Launch counts are printed as `GRADSTORE <case> launches elementwise plain <n> store <m>` (pytest -s)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mcvc_oracle as orc  # noqa: E402
from mask_cyclegan_vc._hip import check, lib, ptr, ptr_table, stream  # noqa: E402
from mask_cyclegan_vc.engine import D_NAMES, G_NAMES, TrainEngine  # noqa: E402
from mask_cyclegan_vc.model import Discriminator, Generator  # noqa: E402
from mask_cyclegan_vc.schedule import StepSchedule  # noqa: E402
from test_hip_model import _launches  # noqa: E402
from test_hip_update import HYPER, _flat_group, _state  # noqa: E402
from test_hip_wino_chunks import N_CHUNKED, _Layer  # noqa: E402

STORE = 4                      # MCVC_BWD_STORE_GRADS
MCVC_ERR_INVALID = 1001
NAN = float("nan")
MODE_GATE = 5e-5               # (see the module docstring)

GEN_SHAPES = [(1, 64), (2, 64), (1, 40), (1, 72), (1, 66)]
DISC_SHAPES = [(1, 64), (2, 64), (2, 72)]
# Shapes at which some covered layer's writer can only add, so that the zero-fill must run.  Generator: downSample2's phase-form Winograd
# weight gradient needs an even input width T / 2 (conv_wgrad: (W & 1) == 0), so T = 66 falls back to the direct kernel; T = 72 does NOT
# (every frame count that is a multiple of 4 keeps all the storing writers: measured 22 "elementwise" launches with and without the
# flag), so (1, 72) is held to the equality alone.  Discriminator: at T = 72 the third stride-2 layer's input is 20 x 9 -- odd, no
# phase-split layout, the staged fall-back.  conv_wgrad zero-fills per tensor: at these shapes between one and (number of covered tensors)
# more launches than the plain pass has, at every other shape exactly as many as the plain pass.
FALLBACK = {("gen", 1, 66), ("disc", 2, 72)}


@pytest.fixture
def deterministic_mode():
    L = lib()
    was = L.mcvc_set_deterministic(1)
    yield
    L.mcvc_set_deterministic(was)


@pytest.fixture
def atomic_mode():
    L = lib()
    was = L.mcvc_set_deterministic(0)
    yield
    L.mcvc_set_deterministic(was)


def _covered(kind):
    buf = (ctypes.c_ubyte * 128)()
    n = lib().mcvc_grad_store_mask(0 if kind == "gen" else 1, 64, buf)
    assert n == (110 if kind == "gen" else 20)
    return [bool(b) for b in buf[:n]]


def _same(a, b):
    """Element-wise == (so -0.0 equals +0.0) and no NaN on either side."""
    return bool((a == b).all())


class _Net(object):
    """One network on the C ABI: parameters, packed weights, workspaces, and forward / backward passes on seeded inputs."""

    def __init__(self, kind, B, T, seed=37):
        L = self.L = lib()
        self.kind, self.B, self.T = kind, B, T
        mod = Generator() if kind == "gen" else Discriminator()
        mod.load_state_dict(orc.filler_params("G" if kind == "gen" else "D", seed), strict=True)
        self.mod = mod.cuda()
        self.ps = list(self.mod.parameters())
        self.live = [not (kind == "disc" and 14 <= i <= 17) for i in range(len(self.ps))]      # (downSample4 takes no part in forward)
        self.cov = _covered(kind)
        self.packed = self.mod.packed_weights(self.ps, force=True) if kind == "gen" else self.mod.packed_weights(self.ps)
        self.tab = ptr_table(self.ps)
        if kind == "gen":
            self.n_scr = L.mcvc_gen_scratch_floats(B, T)
            n_stash = L.mcvc_gen_stash_floats(B, T)
            self.oshape = (B, 80, L.mcvc_gen_out_frames(T))
        else:
            self.n_scr = L.mcvc_disc_scratch_floats(B, T)
            n_stash = L.mcvc_disc_stash_floats(B, T)
            self.oshape = (B, 1, 10, L.mcvc_disc_out_frames(T))
        self.scratch, self.stash = torch.zeros(self.n_scr, device="cuda"), torch.zeros(n_stash, device="cuda")
        if kind == "gen":
            L.mcvc_gen_trunk_fault(ptr(self.scratch), B, T, 1, stream())
        self.mask = torch.ones(B, 80, T)
        self.mask[:, :, 5:11] = 0
        self.mask = self.mask.cuda()
        self.out = torch.empty(self.oshape, device="cuda")

    def inputs(self, seed):
        rng = torch.Generator().manual_seed(seed)
        return torch.randn(self.B, 80, self.T, generator=rng).cuda(), torch.randn(self.oshape, generator=rng).cuda()

    def forward(self, x):
        L = self.L
        if self.kind == "gen":
            check(L.mcvc_gen_forward(self.tab, ptr(self.packed), ptr(x), ptr(self.mask), ptr(self.out), ptr(self.stash), ptr(self.scratch), self.n_scr,
                                     self.B, self.T, stream()), "gen_forward")
        else:
            check(L.mcvc_disc_forward(self.tab, ptr(self.packed), ptr(x), ptr(self.out), ptr(self.stash), ptr(self.scratch), self.n_scr, self.B, self.T,
                                      stream()), "disc_forward")

    def grads(self, poison):
        """Gradient tensors: all zero, or (poison) NaN in the covered tensors and zero in the others -- a store-ready buffer at its worst."""
        out = []
        for p, live, cov in zip(self.ps, self.live, self.cov):
            out.append(None if not live else (torch.full_like(p, NAN) if (poison and cov) else torch.zeros_like(p)))
        return out

    def backward(self, grads, dout, flags):
        L = self.L
        gtab = ptr_table(grads)
        if self.kind == "gen":
            check(L.mcvc_gen_backward_flags(self.tab, ptr(self.packed), gtab, ptr(self.mask), ptr(dout), None, 0, ptr(self.stash), ptr(self.scratch),
                                            self.n_scr, self.B, self.T, stream(), None, None, flags), "gen_backward")
        else:
            check(L.mcvc_disc_backward_flags(self.tab, ptr(self.packed), gtab, ptr(dout), 0, None, 0, ptr(self.stash), ptr(self.scratch), self.n_scr,
                                             self.B, self.T, stream(), None, flags), "disc_backward")

    def one_pass(self, poison, flags, seed=31):
        x, dout = self.inputs(seed)
        self.forward(x)
        g = self.grads(poison)
        self.backward(g, dout, flags)
        torch.cuda.synchronize()
        return g

    def assert_equal(self, got, want, what):
        n_cov = 0
        for i, (a, b) in enumerate(zip(got, want)):
            if a is None:
                assert b is None
                continue
            assert _same(a, b), (what, i, self.cov[i], int((a != b).sum()), a.numel())
            n_cov += int(self.cov[i] and float(b.abs().max()) > 0)
        assert n_cov == sum(self.cov)                      # every covered tensor received a gradient (nothing compared 0 == 0)


@functools.lru_cache(maxsize=None)
def _net(kind, B, T):
    return _Net(kind, B, T)


@functools.lru_cache(maxsize=None)
def _fixed_reference(kind, B, T):
    """The plain pass from an all-zero buffer in deterministic mode: computed once per shape, shared, never written to."""
    L = lib()
    was = L.mcvc_set_deterministic(1)
    try:
        return tuple(_net(kind, B, T).one_pass(False, 0))
    finally:
        L.mcvc_set_deterministic(was)


CASES = [("gen", B, T) for B, T in GEN_SHAPES] + [("disc", B, T) for B, T in DISC_SHAPES]
IDS = ["%s-B%d-T%d" % c for c in CASES]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. one pass stores
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,T", CASES, ids=IDS)
def test_one_store_pass_equals_a_plain_pass_from_zeros(deterministic_mode, kind, B, T):
    net = _net(kind, B, T)
    want = _fixed_reference(kind, B, T)
    got = net.one_pass(True, STORE)
    net.assert_equal(got, want, "store")
    # which writers ran: a zero-fill is one more "elementwise" launch than the plain pass has
    x, dout = net.inputs(31)
    net.forward(x)
    plain = _launches("elementwise", lambda: net.backward(net.grads(False), dout, 0))
    store = _launches("elementwise", lambda: net.backward(net.grads(True), dout, STORE))
    print("GRADSTORE %s-B%d-T%d launches elementwise plain %d store %d" % (kind, B, T, plain, store))
    if (kind, B, T) in FALLBACK:
        assert 1 <= store - plain <= sum(net.cov), (plain, store)          # the zero-fill path did trigger: at most once per covered tensor
    else:
        assert store == plain, (plain, store)                              # ... and nowhere else


@pytest.mark.parametrize("name", ["f25", "f23-phase"])
def test_a_winograd_pass_in_several_chunks_stores_once(deterministic_mode, name):
    """Three samples of 5550 tiles run as chunks of 2 + 1 (tests/test_hip_wino_chunks.py): the first chunk stores, the second adds to it."""
    layer = _Layer(name, N_CHUNKED)
    layer.fresh_scratch()

    def wgrad(fill, flags):
        dws = [torch.full_like(w, fill) for w in layer.wd]
        check(layer.L.mcvc_layer_wgrad_flags(ptr(layer.xd), ptr(layer.dyd), ptr(dws[0]), ptr(dws[1]) if layer.nbr == 2 else None, ptr(layer.scratch),
                                             layer.n_scr, *layer.dims, *layer.spec, layer.scheme, flags, stream()), "layer_wgrad_flags")
        return dws
    want, got = wgrad(0.0, 0), wgrad(NAN, STORE)
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert _same(a, b) and float(b.abs().max()) > 0, (name, int((a != b).sum()))
    assert _launches("wino_gemm", lambda: wgrad(NAN, STORE)) == 2          # two chunks did run
    assert layer.L.mcvc_layer_wgrad_flags(ptr(layer.xd), ptr(layer.dyd), ptr(want[0]), ptr(want[1]) if layer.nbr == 2 else None, ptr(layer.scratch),
                                          layer.n_scr, *layer.dims, *layer.spec, layer.scheme, 1, stream()) == MCVC_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the second pass still accumulates
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,T", [("gen", 1, 64), ("gen", 1, 72), ("disc", 1, 64), ("disc", 2, 72)])
def test_a_plain_pass_behind_a_store_pass_accumulates(deterministic_mode, kind, B, T):
    net = _net(kind, B, T)
    (x1, d1), (x2, d2) = net.inputs(31), net.inputs(47)

    def two_passes(poison, first_flags):
        g = net.grads(poison)
        net.forward(x1)
        net.backward(g, d1, first_flags)
        net.forward(x2)
        net.backward(g, d2, 0)
        torch.cuda.synchronize()
        return g
    want, got = two_passes(False, 0), two_passes(True, STORE)
    net.assert_equal(got, want, "store + plain")
    one = _fixed_reference(kind, B, T)
    moved = sum(1 for a, b, c in zip(want, one, net.cov) if c and not _same(a, b))
    assert moved == sum(net.cov)                           # (the second pass did add something to every covered tensor)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. default mode (atomics on)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,T", CASES, ids=IDS)
def test_store_pass_in_default_mode(atomic_mode, kind, B, T):
    net = _net(kind, B, T)
    want = _fixed_reference(kind, B, T)
    got = net.one_pass(True, STORE)
    for i, (a, b) in enumerate(zip(got, want)):
        if a is None or not net.cov[i]:
            continue
        assert bool(torch.isfinite(a).all()), i
        e = float((a.double() - b.double()).norm() / b.double().norm())
        print("GRADSTORE %s-B%d-T%d default-mode param %d rel %.3g gate %.3g" % (kind, B, T, i, e, MODE_GATE))
        assert e < MODE_GATE, (i, e)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. update mode 2
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gen", "disc"])
def test_update_mode_2_equals_mode_1_and_leaves_the_covered_gradients(kind):
    L = lib()
    T, max_batch = 64, 2
    mod = Generator() if kind == "gen" else Discriminator()
    mod.load_state_dict(orc.filler_params("G" if kind == "gen" else "D", 11), strict=True)
    mod = mod.cuda()
    names = [k for k, _ in mod.named_parameters()]
    live = [i for i, k in enumerate(names) if "downSample4" not in k]
    ps, flat, offs = _flat_group(mod, live)
    tab = ptr_table(ps)
    numel = (ctypes.c_longlong * len(ps))(*[(p.numel() if i in offs else 0) for i, p in enumerate(ps)])
    n = flat.numel()
    grad, grad2, m, v = _state(n, 5, ps, offs)
    h = HYPER
    n_packed = L.mcvc_gen_packed_floats() if kind == "gen" else L.mcvc_disc_packed_floats()

    def update(mode, masks, g2=None, gr=None):
        keep = flat.clone()
        gr = grad.clone() if gr is None else gr
        mm, vv = m.clone(), v.clone()
        packed = torch.zeros(n_packed, device="cuda")
        rcs = []
        for mask in masks:
            if kind == "gen":
                rcs.append(L.mcvc_gen_update_ranges(tab, numel, ptr(packed), max_batch, T, mask, ptr(flat), ptr(gr), ptr(g2), ptr(mm), ptr(vv),
                                                    h["lr"], h["b1"], h["b2"], h["eps"], h["step"], h["scale"], mode, stream()))
            else:
                rcs.append(L.mcvc_disc_update_batch(tab, numel, ptr(packed), max_batch, T, ptr(flat), ptr(gr), ptr(g2), ptr(mm), ptr(vv),
                                                    h["lr"], h["b1"], h["b2"], h["eps"], h["step"], h["scale"], mode, stream()))
        torch.cuda.synchronize()
        f = flat.clone()
        flat.copy_(keep)
        return rcs, f, gr, mm, vv, packed

    cov = _covered(kind)
    for masks in ([7], [1, 2, 8, 16, 32]) if kind == "gen" else ([7],):
        one, two = update(1, masks), update(2, masks)
        assert one[0] == [0] * len(masks) and two[0] == [0] * len(masks)
        for name, a, b in zip(("parameters", "grad", "exp_avg", "exp_avg_sq", "packed"), one[1:], two[1:]):
            if name != "grad":
                assert torch.equal(a, b), (masks, name, int((a != b).sum()))
        assert not torch.equal(two[1], flat)
        assert float(one[2].abs().max()) == 0.0                                   # mode 1: everything cleared
        for i in live:                                                            # mode 2: exactly the masked tensors are left alone
            sl = slice(offs[i], offs[i] + ps[i].numel())
            if cov[i]:
                assert torch.equal(two[2][sl], grad[sl]) and float(grad[sl].abs().max()) > 0, names[i]
            else:
                assert float(two[2][sl].abs().max()) == 0.0, names[i]
    # mode 2 has one gradient buffer; other modes do not exist
    gr = grad.clone()
    for mode, g2 in ((2, grad2.clone()), (3, None), (-1, None)):
        rcs = update(mode, [7], g2=g2, gr=gr)[0]
        assert rcs == [MCVC_ERR_INVALID], (mode, rcs)
    assert torch.equal(gr, grad)                                                  # (a refused call did nothing)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. the engine: grad_store on and off
# ---------------------------------------------------------------------------------------------------------------------------------------
def _engine_nets(seed0):
    nets = {}
    for i, n in enumerate(orc.NET_ORDER):
        mdl = Generator() if i < 2 else Discriminator()
        mdl.load_state_dict(orc.filler_params("G" if i < 2 else "D", seed0 + i), strict=True)
        nets[n] = mdl.cuda()
    return nets


def _batch(B, seed):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(2):
        out.append(torch.from_numpy(rs.randn(B, 80, 64).astype(np.float32)).cuda())
        out.append(torch.from_numpy(orc.fif_mask(rs, B, 80, 64, 25)).cuda())
    return out


def _poison_covered(eng):
    """NaN into every covered gradient of all six networks (through the parameters' own gradient views)."""
    for names, kind in ((G_NAMES, "gen"), (D_NAMES, "disc")):
        cov = _covered(kind)
        for n in names:
            for c, p in zip(cov, eng.nets[n].parameters()):
                if c and p.grad is not None:
                    p.grad.fill_(NAN)


def _engine(store, B, stop_identity_after=1e4, grouped_max_b=None):
    nets = _engine_nets(700)
    eng = TrainEngine(nets, B, 64, schedule=StepSchedule(batch_size=B, n_samples=4 * B, stop_identity_after=stop_identity_after))
    eng.grad_store = store
    eng.merged = False
    if grouped_max_b is not None:
        eng.grouped_max_b = grouped_max_b
    return nets, eng


@functools.lru_cache(maxsize=None)
def _five_steps(store, B=1, lagged=False, stop_identity_after=1e4, flush_after=None, poison=False, grouped_max_b=None):
    nets, eng = _engine(store, B, stop_identity_after, grouped_max_b)
    p0 = [p.detach().clone() for n in G_NAMES + D_NAMES for p in nets[n].parameters()]
    if grouped_max_b is not None:
        assert eng._use_pipeline() and B >= eng.split_d_min_batch          # (the pipelined schedule with split discriminator halves)
    losses = []
    for it in range(5):
        eng.step(*_batch(B, 900 + it))
        lo = eng.losses(lagged=2) if lagged else eng.losses()
        losses.append(None if lo is None else tuple(sorted(lo.items())))
        if flush_after is not None and it + 1 == flush_after:
            eng.flush()
            if poison:
                torch.cuda.synchronize()
                _poison_covered(eng)
    losses.append(tuple(sorted(eng.losses().items())))          # completes the last step (a pending discriminator phase included)
    eng.flush()
    torch.cuda.synchronize()
    params = [p.detach().clone() for n in G_NAMES + D_NAMES for p in eng.nets[n].parameters()]
    assert sum(1 for a, b in zip(params, p0) if not torch.equal(a, b)) > 100          # (the steps did move the parameters)
    del eng
    return losses, params


def _assert_runs_equal(on, off, what):
    assert on[0] == off[0], (what, on[0], off[0])
    assert all(np.isfinite(v) for lo in on[0] if lo is not None for _, v in lo), (what, on[0])
    for i, (a, b) in enumerate(zip(on[1], off[1])):
        assert bool(torch.isfinite(a).all()) and _same(a, b), (what, i, int((a != b).sum()))


ENGINE_VARIANTS = {
    "sync-losses": dict(),
    "unflushed": dict(lagged=True),
    "identity-cut-off": dict(lagged=True, stop_identity_after=0),
    "flush-after-2": dict(lagged=True, flush_after=2),
    # the grouped / pipelined schedule enabled at B = 8 (the default leaves it at 4 samples, where the discriminator passes are not yet
    # split): real1 / real2 run with the store flag, fake1 / fake2 add to what they stored
    "B8-split-halves": dict(B=8, lagged=True, grouped_max_b=8),
    "B5-above-grouped": dict(B=5),          # four-lane schedule throughout: mode-1 updates, no store pass
}


@pytest.mark.parametrize("variant", sorted(ENGINE_VARIANTS))
def test_engine_steps_are_equal_with_grad_store_on_and_off(deterministic_mode, variant):
    kw = ENGINE_VARIANTS[variant]
    on, off = _five_steps(True, **kw), _five_steps(False, **kw)
    _assert_runs_equal(on, off, variant)


@pytest.mark.parametrize("B", [1, 8])
def test_engine_never_reads_a_stale_covered_gradient(deterministic_mode, B):
    """After step 2 and a flush() every covered gradient is overwritten with NaN: the store passes of the following steps must not read
    them -- the remaining steps stay finite and equal to the run without store mode.  B = 8 (grouped schedule enabled there): the real
    halves of the split discriminator passes store, the fake halves add -- if both stored, the real halves' gradients would be lost; if
    neither did, the NaN would spread."""
    kw = dict(B=B, lagged=True, flush_after=2, grouped_max_b=8 if B == 8 else None)
    on = _five_steps(True, poison=True, **kw)
    off = _five_steps(False, **kw)
    _assert_runs_equal(on, off, "poisoned B=%d" % B)


# A store-ready buffer met by a path that cannot store: two pipelined steps at B = 1 and a flush() leave both gradient buffers store-ready
# (asserted); the covered gradients are then overwritten with NaN and the engine goes on with something that only accumulates, which
# must therefore zero the buffers first (engine._take_grads).
FALLBACK_PATHS = ["B5-step", "four-lane-step", "four-lane-phases", "grouped-phases"]


@functools.lru_cache(maxsize=None)
def _then(store, path):
    nets, eng = _engine(store, 1)
    for it in range(2):
        eng.step(*_batch(1, 900 + it))
    eng.flush()
    torch.cuda.synchronize()
    assert (eng._g_grad_ready, eng._d_grad_ready) == (store, store) and (eng._g_grad_clean, eng._d_grad_clean) == (not store, not store)
    if store:
        _poison_covered(eng)
        assert not bool(torch.isfinite(eng.g_group.grad).all()) and not bool(torch.isfinite(eng.d_group.grad).all())
    if path in ("B5-step", "four-lane-step"):
        B = 5 if path == "B5-step" else 1
        if path == "four-lane-step":
            eng.grouped = False                                # a schedule change behind a flush()
        assert B > eng.grouped_max_b or not eng.grouped
        eng.step(*_batch(B, 950))
        out = [tuple(sorted(eng.losses().items()))]
        eng.flush()
        out += [p.detach().clone() for n in G_NAMES + D_NAMES for p in eng.nets[n].parameters()]
    else:
        # a phase called on its own leaves its gradients in the flat buffers (no update): the four-lane phases zero a store-ready buffer,
        # the grouped ones store into it
        inp = _batch(1, 950)
        if path == "four-lane-phases":
            eng.grouped = False
            eng.generator_phase(*inp)
            eng.discriminator_phase(*inp)
        else:
            eng.generator_phase_grouped(*inp)
            eng.discriminator_phase_grouped(*inp)
        out = [tuple(eng.slots.tolist()), eng.g_group.grad.detach().clone(), eng.d_group.grad.detach().clone()]
    torch.cuda.synchronize()
    eng.check_faults()
    del eng
    return out


@pytest.mark.parametrize("path", FALLBACK_PATHS)
def test_a_path_that_cannot_store_zeroes_a_store_ready_buffer(deterministic_mode, path):
    on, off = _then(True, path), _then(False, path)
    assert on[0] == off[0] and all(np.isfinite(v if isinstance(v, float) else v[1]) for v in on[0]), (path, on[0], off[0])
    for i, (a, b) in enumerate(zip(on[1:], off[1:])):
        assert bool(torch.isfinite(a).all()) and _same(a, b), (path, i, int((a != b).sum()))
        assert path.endswith("-step") or float(b.abs().max()) > 0, (path, i)          # (the phases did leave gradients to compare)
