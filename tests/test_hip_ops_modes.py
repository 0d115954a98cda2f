"""GPU: op-level parity of the fixed-order (deterministic) launch plans and of accumulation into non-zero destinations.

tests/test_hip_ops.py runs every kernel in the default (atomic) mode and accumulates into zeros.  Here the same entry points of the C ABI
(include/mcvc.h) run under BOTH settings of mcvc_set_deterministic -- the fixed-order plans are other code: slab K splits folded by
wgrad_reduce_kernel, one-chunk walks of the few-channel weight gradients, one sample chunk in the InstanceNorm backward -- and every
destination the header documents as `+=` is also pre-filled with seeded noise of the increment's rms (a store in place of an add is then an
error of about 1), every plain-store destination with NaN.  References are plain PyTorch on the CPU in float64 from the same fp32 inputs;
the gates are those of tests/test_hip_ops.py (2e-5 direct convolutions, 5e-5 layer ops / trunk backward, 5e-5 | 2e-4 InstanceNorm forward |
gradients).  In "fixed" mode every op runs twice into fresh destinations and the two results must be bit-equal.

Every measured distance is printed as a line `MODES <family> <mode> <what> <distance> <gate>` before it is asserted (pytest -s shows them)."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import mcvc_oracle as orc  # noqa: E402  (parameter filler only)
from mask_cyclegan_vc import ops  # noqa: E402
from mask_cyclegan_vc._hip import check, lib, ptr, ptr_table, stream  # noqa: E402
from mask_cyclegan_vc.model import Discriminator, Generator  # noqa: E402
from test_hip_ops import CONV_CASES, LAYER_CASES, rel_l2  # noqa: E402

MAX_SLABS = 16
NAN = float("nan")

# (name, Cin, Cout, KH, KW, stride, ph, pw, N, H, W, shuffle): the table of tests/test_hip_ops.py + two weight tensors whose size leaves the
# other two remainders modulo 4 (891 = 4 * 222 + 3 floats, 630 = 4 * 157 + 2) for the reduce kernel's scalar tail
CONV = {c[0]: c for c in CONV_CASES}
CONV["dw891"] = ("dw891", 3, 33, 3, 3, 1, 1, 1, 2, 9, 7, False)
CONV["dw630"] = ("dw630", 6, 35, 1, 3, 1, 0, 1, 2, 5, 20, False)
LAYER = {"%s-s%d" % (c[0], s): (c, s) for c in LAYER_CASES for s in c[-1]}


@pytest.fixture(params=("atomic", "fixed"))
def mode(request):
    L = lib()
    was = L.mcvc_set_deterministic(1 if request.param == "fixed" else 0)
    try:
        yield request.param
    finally:
        L.mcvc_set_deterministic(was)


def _run(mode, fn):
    """fn() allocates fresh destinations, launches and returns a dict of result tensors.  Fixed mode: twice, bit-equal."""
    out = fn()
    torch.cuda.synchronize()
    if mode == "fixed":
        again = fn()
        torch.cuda.synchronize()
        for k in out:
            assert torch.equal(out[k], again[k]), "fixed-order mode: two runs of %s differ" % k
    return out


def _prefill(ref, fill, seed):
    """The initial value of a `+=` destination: zeros, or seeded noise scaled to the rms of the fp64 reference increment."""
    if not fill:
        return torch.zeros(ref.shape)
    r = torch.randn(ref.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    r *= ref.double().pow(2).mean().sqrt() / r.pow(2).mean().sqrt()
    return r.float()


def _dev(t, offset=0):
    """A device copy of t; offset = 1 puts it one float into a 16-byte aligned allocation."""
    base = torch.empty(t.numel() + 8, device="cuda")
    assert base.data_ptr() % 16 == 0
    d = base[offset:offset + t.numel()].view(t.shape)
    d.copy_(t)
    return d


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _gate(family, mode, what, got, pre, ref, gate):
    """rel_l2(got - prefill, fp64 increment) < gate; a NaN anywhere fails it."""
    inc = got.detach().double().cpu() - (pre.double() if pre is not None else 0.0)
    e = rel_l2(inc, ref)
    print("MODES %s %s %s %.3e %.1e" % (family, mode, what, e, gate))
    assert e < gate, (family, mode, what, e, gate)
    return e


# ---------------------------------------------------------------------------------------------------------------------------------------
# direct convolutions: weight gradient (generic kernel: atomic | slabs + wgrad_reduce_kernel; few-channel kernels; small-K), bias gradient,
# data gradient, forward
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_data(name):
    _, Cin, Cout, KH, KW, s, ph, pw, N, H, W, sh = CONV[name]
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, KH, KW, generator=g) / np.sqrt(Cin * KH * KW)
    b = torch.randn(Cout, generator=g)
    OH, OW = (H + 2 * ph - KH) // s + 1, (W + 2 * pw - KW) // s + 1
    dy = torch.randn(N, Cout, OH, OW, generator=torch.Generator().manual_seed(5))
    return x, w, b, dy


@functools.lru_cache(maxsize=None)
def _conv_ref(name, what):
    _, Cin, Cout, KH, KW, s, ph, pw, N, H, W, sh = CONV[name]
    x, w, b, dy = (t.double() for t in _conv_data(name))
    if what == "fwd":
        return F.conv2d(x, w, b, s, (ph, pw))
    if what == "dgrad":
        return torch.nn.grad.conv2d_input(x.shape, w, dy, s, (ph, pw))
    return torch.nn.grad.conv2d_weight(x, w.shape, dy, s, (ph, pw))


# the generic kernel's slab K split (fixed mode; in atomic mode these take the atomic tiny-dW path): aligned dw -> float4 reduce + scalar tail,
# dw one float into an aligned allocation -> the scalar reduce
SLAB_CASES = ["ragged.s1", "ragged.s2", "ragged.wide", "dw891", "dw630"]
# cin2 (bands of 2 and 4), cout1 on the matrix cores (partial channel rounds, short last band), cout1 VALU (1 x 3), all with N >= 2;
# the generic kernel's lane mode (d.conv1: Cin = 1); small-K; d.ds2: 1.2 M floats, the slab path in both modes
OTHER_WGRAD = ["g.conv1", "ragged.conv1", "g.last", "ragged.last", "d.out", "d.conv1", "g.res_vg", "g.2dto1d", "d.ds2"]
WGRAD_PARAMS = [(n, o) for n in SLAB_CASES for o in (0, 1)] + [(n, 0) for n in OTHER_WGRAD]


@pytest.mark.parametrize("fill", [False, True], ids=["zeros", "filled"])
@pytest.mark.parametrize("name,offset", WGRAD_PARAMS, ids=["%s-off%d" % p for p in WGRAD_PARAMS])
def test_conv_wgrad(mode, name, offset, fill):
    L = lib()
    _, Cin, Cout, KH, KW, s, ph, pw, N, H, W, sh = CONV[name]
    x, w, b, dy = _conv_data(name)
    ref = _conv_ref(name, "wgrad")
    n_slab = L.mcvc_conv2d_wgrad_slab_floats(N, Cin, H, W, Cout, KH, KW, s, ph, pw)
    if name in SLAB_CASES or name == "d.ds2":
        assert n_slab > 0, "%s plans no K split: the reduce kernel would not run" % name
        assert ref.numel() % 4 == {"ragged.s1": 1, "ragged.s2": 0, "ragged.wide": 0, "dw891": 3, "dw630": 2, "d.ds2": 0}[name]
    pre = _prefill(ref, fill, 100 + offset)
    xd, dyd = x.cuda(), dy.cuda()

    def fn():
        dw = _dev(pre, offset)
        assert dw.data_ptr() % 16 == 4 * offset
        slabs = _nan(n_slab) if n_slab > 0 else None
        check(L.mcvc_conv2d_wgrad(ptr(xd), ptr(dyd), ptr(dw), ptr(slabs), n_slab, N, Cin, H, W, Cout, KH, KW, s, ph, pw, stream()), "conv2d_wgrad")
        return {"dw": dw}
    out = _run(mode, fn)
    _gate("conv_wgrad", mode, "%s-off%d-%s" % (name, offset, "filled" if fill else "zeros"), out["dw"], pre, ref, 2e-5)


@pytest.mark.parametrize("fill", [False, True], ids=["zeros", "filled"])
def test_cin1_wgrad_through_the_planner(mode, fill):
    """wgrad_cin1_kernel is reached only through the planner (conv_wgrad): d.conv1 as a layer, N = 2 -> several (sample, band) units."""
    L = lib()
    _, Cin, Cout, KH, KW, s, ph, pw, N, H, W, sh = CONV["d.conv1"]
    x, w, b, dy = _conv_data("d.conv1")
    ref = _conv_ref("d.conv1", "wgrad")
    spec = (Cin, Cout, 1, KH, KW, s, ph, pw)
    n_scr = L.mcvc_layer_scratch_floats(N, H, W, *spec)
    assert n_scr > 0
    pre = _prefill(ref, fill, 110)
    xd, dyd = x.cuda(), dy.cuda()

    def fn():
        dw = _dev(pre)
        scratch = torch.zeros(n_scr, device="cuda")
        check(L.mcvc_layer_wgrad(ptr(xd), ptr(dyd), ptr(dw), None, ptr(scratch), n_scr, N, H, W, *spec, 3, stream()), "layer_wgrad")
        return {"dw": dw}
    out = _run(mode, fn)
    _gate("conv_wgrad", mode, "d.conv1-planner-%s" % ("filled" if fill else "zeros"), out["dw"], pre, ref, 2e-5)


@pytest.mark.parametrize("fill", [False, True], ids=["zeros", "filled"])
@pytest.mark.parametrize("C,N,P", [(33, 3, 35), (256, 2, 5120)])
def test_bias_grad(mode, C, N, P, fill):
    L = lib()
    dy = torch.randn(N, C, P, generator=torch.Generator().manual_seed(21))
    ref = dy.double().sum((0, 2))
    pre = _prefill(ref, fill, 120)
    dyd = dy.cuda()

    def fn():
        db = _dev(pre)
        check(L.mcvc_bias_grad(ptr(dyd), ptr(db), N, C, P, stream()), "bias_grad")
        return {"db": db}
    out = _run(mode, fn)
    _gate("bias_grad", mode, "C%d-N%d-P%d-%s" % (C, N, P, "filled" if fill else "zeros"), out["db"], pre, ref, 2e-5)


@pytest.mark.parametrize("name", ["ragged.s2", "ragged.s1", "g.ds2", "trunk.T4"])
def test_conv_forward_and_dgrad(mode, name):
    L = lib()
    _, Cin, Cout, KH, KW, s, ph, pw, N, H, W, sh = CONV[name]
    x, w, b, dy = _conv_data(name)
    xd, wd, bd, dyd = x.cuda(), w.cuda(), b.cuda(), dy.cuda()
    n_pack = L.mcvc_conv2d_pack_floats(Cout, Cin, KH, KW)

    def fn():
        y, dx = _nan(*dy.shape), _nan(*x.shape)
        wpack = torch.zeros(n_pack, device="cuda")
        slabs = _nan((MAX_SLABS - 1) * max(y.numel(), dx.numel()))
        check(L.mcvc_conv2d_forward(ptr(xd), ptr(wd), ptr(bd), ptr(y), ptr(wpack), ptr(slabs), MAX_SLABS, N, Cin, H, W, Cout, KH, KW, s, ph, pw,
                                    0, stream()), "conv2d_forward")
        wpack2 = torch.zeros(n_pack, device="cuda")
        check(L.mcvc_conv2d_dgrad(ptr(dyd), ptr(wd), ptr(dx), ptr(wpack2), ptr(slabs), MAX_SLABS, N, Cin, H, W, Cout, KH, KW, s, ph, pw, stream()),
              "conv2d_dgrad")
        return {"y": y, "dx": dx}
    out = _run(mode, fn)
    _gate("conv_fwd", mode, name, out["y"], None, _conv_ref(name, "fwd"), 2e-5)
    _gate("conv_dgrad", mode, name, out["dx"], None, _conv_ref(name, "dgrad"), 2e-5)


# ---------------------------------------------------------------------------------------------------------------------------------------
# one convolution layer through the planner: Winograd (2x2 and 4x4 tiles), two-branch stride-2 layers, implicit GEMMs with a K split
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layer_data(key):
    c, scheme = LAYER[key]
    name, Cin, Cout, nbr, KH, KW, s, ph, pw, N, H, W, shuffle, _ = c
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, Cin, H, W, generator=g)
    ws = [torch.randn(Cout, Cin, KH, KW, generator=g) / np.sqrt(Cin * KH * KW) for _ in range(nbr)]
    bs = [torch.randn(Cout, generator=g) for _ in range(nbr)]
    wcat, bcat = torch.cat(ws, 0).double(), torch.cat(bs, 0).double()
    y = F.conv2d(x.double(), wcat, bcat, stride=s, padding=(ph, pw))
    dy = torch.randn(y.shape, generator=g)
    dx = torch.nn.grad.conv2d_input(x.shape, wcat, dy.double(), stride=s, padding=(ph, pw))
    dw = torch.nn.grad.conv2d_weight(x.double(), wcat.shape, dy.double(), stride=s, padding=(ph, pw))
    return x, ws, bs, dy, (F.pixel_shuffle(y, 2) if shuffle else y), dx, [dw[i * Cout:(i + 1) * Cout] for i in range(nbr)]


@pytest.mark.parametrize("fill", [False, True], ids=["zeros", "filled"])
@pytest.mark.parametrize("key", ["up2.ragged-s1", "ds1.ragged-s1", "d.ds1.small-s5", "d.ds1.B4-s5", "up2.T48-s2"])
def test_layer_ops(mode, key, fill):
    L = lib()
    c, scheme = LAYER[key]
    name, Cin, Cout, nbr, KH, KW, s, ph, pw, N, H, W, shuffle, _ = c
    x, ws, bs, dy, y_ref, dx_ref, dw_ref = _layer_data(key)
    spec = (Cin, Cout, nbr, KH, KW, s, ph, pw)
    n_scr = L.mcvc_layer_scratch_floats(N, H, W, *spec)
    packed = torch.zeros(L.mcvc_layer_packed_floats(*spec), device="cuda")
    wd, bd = [w.cuda() for w in ws], [b.cuda() for b in bs]
    w1, b1 = (wd[1], bd[1]) if nbr == 2 else (None, None)
    check(L.mcvc_layer_pack(ptr(wd[0]), ptr(bd[0]), ptr(w1), ptr(b1), ptr(packed), *spec, stream()), "layer_pack")
    xd, dyd = x.cuda(), dy.cuda()
    pres = [_prefill(r, fill, 130 + i) for i, r in enumerate(dw_ref)]

    def fn():
        scratch = torch.zeros(n_scr, device="cuda")
        y, dx = _nan(*y_ref.shape), _nan(*x.shape)
        check(L.mcvc_layer_forward(ptr(xd), ptr(packed), ptr(wd[0]), ptr(w1), ptr(y), ptr(scratch), n_scr, N, H, W, *spec, scheme,
                                   1 if shuffle else 0, stream()), "layer_forward")
        check(L.mcvc_layer_dgrad(ptr(dyd), ptr(packed), ptr(wd[0]), ptr(w1), ptr(dx), ptr(scratch), n_scr, N, H, W, *spec, scheme, stream()), "layer_dgrad")
        dws = [_dev(p) for p in pres]
        check(L.mcvc_layer_wgrad(ptr(xd), ptr(dyd), ptr(dws[0]), ptr(dws[1]) if nbr == 2 else None, ptr(scratch), n_scr, N, H, W, *spec, scheme,
                                 stream()), "layer_wgrad")
        out = {"y": y, "dx": dx}
        out.update({"dw%d" % i: d for i, d in enumerate(dws)})
        return out
    out = _run(mode, fn)
    tag = "%s-%s" % (key, "filled" if fill else "zeros")
    _gate("layer_fwd", mode, tag, out["y"], None, y_ref, 5e-5)
    _gate("layer_dgrad", mode, tag, out["dx"], None, dx_ref, 5e-5)
    for i in range(nbr):
        _gate("layer_wgrad", mode, "%s-dw%d" % (tag, i), out["dw%d" % i], pres[i], dw_ref[i], 5e-5)


# ---------------------------------------------------------------------------------------------------------------------------------------
# InstanceNorm + activation, forward and backward (register kernels, P <= 5120; the generic kernels, P = 5184)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _norm_ref(x, gamma, beta, gamma_g, beta_g, res, act, C):
    if act == ops.ACT_GLU:
        a = F.instance_norm(x[:, :C], None, None, gamma, beta, True, 0.0, 1e-5)
        g = F.instance_norm(x[:, C:], None, None, gamma_g, beta_g, True, 0.0, 1e-5)
        y = a * torch.sigmoid(g)
    else:
        z = F.instance_norm(x, None, None, gamma, beta, True, 0.0, 1e-5)
        y = z * torch.sigmoid(z) if act == ops.ACT_SILU else z
    return y if res is None else y + res


def _norm_pipeline(inputs, act, C, dtype):
    """y and the gradients (dx, dgamma, dbeta [, dgamma_gate, dbeta_gate]) of the plain PyTorch pipeline evaluated in `dtype`."""
    x, gamma, beta, gg, bg, res, dy = inputs
    leaves = [t.to(dtype).requires_grad_(True) if t is not None else None for t in (x, gamma, beta, gg, bg)]
    y = _norm_ref(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], res.to(dtype) if res is not None else None, act, C)
    grads = torch.autograd.grad(y, [t for t in leaves if t is not None], dy.to(dtype))
    return y.detach(), [g_.detach() for g_ in grads]


def _norm_inputs(N, C, H, W, act, res, offset_sigmas=0.0):
    g = torch.Generator().manual_seed(11)
    Cx = 2 * C if act == ops.ACT_GLU else C
    if offset_sigmas:          # a per-channel DC offset of that many standard deviations
        sign = (torch.randint(0, 2, (Cx,), generator=g) * 2 - 1).float().view(1, Cx, 1, 1)
        x = torch.randn(N, Cx, H, W, generator=g) + offset_sigmas * sign
    else:
        x = torch.randn(N, Cx, H, W, generator=g) * 1.7 + 0.3
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    gg = 1 + 0.3 * torch.randn(C, generator=g) if act == ops.ACT_GLU else None
    bg = 0.3 * torch.randn(C, generator=g) if act == ops.ACT_GLU else None
    r = torch.randn(N, C, H, W, generator=g) if res else None
    dy = torch.randn(N, C, H, W, generator=g)
    return x, gamma, beta, gg, bg, r, dy


def _norm_launch(L, inputs, N, C, H, W, act, pres):
    """Forward into NaN-filled y / stats, backward into a NaN-filled dx and the pre-filled parameter gradients."""
    x, gamma, beta, gg, bg, r, dy = inputs
    dev = [t.cuda() if t is not None else None for t in (x, gamma, beta, gg, bg, r)]
    y, stats = _nan(N, C, H, W), _nan(N, x.shape[1], 2)
    check(L.mcvc_instnorm_act_forward(ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), ptr(dev[4]), ptr(dev[5]), ptr(y), ptr(stats),
                                      N, C, H, W, act, stream()), "instnorm_act_forward")
    dyd, dx = dy.cuda(), _nan(*x.shape)
    dps = [_dev(p) for p in pres]
    dgg, dbg = (dps[2], dps[3]) if act == ops.ACT_GLU else (None, None)
    check(L.mcvc_instnorm_act_backward(ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), ptr(dev[4]), ptr(stats), ptr(dyd), ptr(dx),
                                       ptr(dps[0]), ptr(dps[1]), ptr(dgg), ptr(dbg), N, C, H, W, act, stream()), "instnorm_act_backward")
    out = {"y": y, "dx": dx}
    out.update({"dp%d" % i: d for i, d in enumerate(dps)})
    return out


NORM_CASES = [  # (N, C, H, W, act, residual)
    (3, 512, 1, 16, ops.ACT_GLU, False), (2, 7, 3, 5, ops.ACT_GLU, False), (2, 1024, 10, 8, ops.ACT_SILU, False),
    (5, 64, 1, 16, ops.ACT_NONE, True),                # N = 5: four unequal sample chunks in atomic mode, one in fixed mode
    (1, 8, 81, 64, ops.ACT_SILU, False), (2, 6, 81, 64, ops.ACT_GLU, False),      # P = 5184 > 5120: norm_fwd_kernel / norm_bwd_kernel
]


@pytest.mark.parametrize("fill", [False, True], ids=["zeros", "filled"])
@pytest.mark.parametrize("N,C,H,W,act,res", NORM_CASES, ids=["%dx%dx%dx%d-a%d-r%d" % c for c in NORM_CASES])
def test_instnorm_act(mode, N, C, H, W, act, res, fill):
    L = lib()
    inputs = _norm_inputs(N, C, H, W, act, res)
    y_ref, g_ref = _norm_pipeline(inputs, act, C, torch.float64)
    pres = [_prefill(r, fill, 140 + i) for i, r in enumerate(g_ref[1:])]
    out = _run(mode, lambda: _norm_launch(L, inputs, N, C, H, W, act, pres))
    tag = "%dx%dx%dx%d-a%d-%s" % (N, C, H, W, act, "filled" if fill else "zeros")
    _gate("norm_fwd", mode, tag, out["y"], None, y_ref, 5e-5)
    _gate("norm_bwd", mode, tag + "-dx", out["dx"], None, g_ref[0], 2e-4)
    for i, (p, r) in enumerate(zip(pres, g_ref[1:])):
        _gate("norm_bwd", mode, "%s-dp%d" % (tag, i), out["dp%d" % i], p, r, 2e-4)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fused backward of one 1-D trunk layer
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trunk_bwd_data(B, T4, Cin, Cout, glu):
    g = torch.Generator().manual_seed(9)
    KW = 3
    f32 = {"x": torch.randn(B, Cin, T4, generator=g)}
    mk = lambda: torch.randn(Cout, Cin, KW, generator=g) / (Cin * KW) ** 0.5      # noqa: E731
    f32["w"], f32["wg"] = mk(), mk()
    f32["b"], f32["bg"] = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    f32["ga"], f32["be"] = 1 + 0.1 * torch.randn(Cout, generator=g), 0.1 * torch.randn(Cout, generator=g)
    f32["gg"], f32["bgt"] = 1 + 0.1 * torch.randn(Cout, generator=g), 0.1 * torch.randn(Cout, generator=g)
    f32["dy"] = torch.randn(B, Cout, T4, generator=g)
    d = {k: v.double().requires_grad_(k in ("x", "w", "wg", "ga", "be", "gg", "bgt")) for k, v in f32.items()}
    c0 = F.conv1d(d["x"], d["w"], d["b"], padding=1)
    c0.retain_grad()
    z = F.instance_norm(c0, weight=d["ga"], bias=d["be"], eps=1e-5)
    if glu:
        c1 = F.conv1d(d["x"], d["wg"], d["bg"], padding=1)
        c1.retain_grad()
        y = z * torch.sigmoid(F.instance_norm(c1, weight=d["gg"], bias=d["bgt"], eps=1e-5))
        conv = torch.cat((c0, c1), 1)
    else:
        y, conv = z, c0
    y.backward(d["dy"])
    conv = conv.detach()
    stats = torch.stack((conv.mean(2), 1.0 / torch.sqrt(conv.var(2, unbiased=False) + 1e-5)), 2).float().contiguous()       # [B][Cx][2]
    tl = lambda t: t.detach().permute(1, 0, 2).contiguous()          # noqa: E731  trunk layout [C][B][T4]
    ref = {"dconv": tl(torch.cat((c0.grad, c1.grad), 1) if glu else c0.grad), "dx": tl(d["x"].grad), "dga": d["ga"].grad, "dbe": d["be"].grad,
           "dw": d["w"].grad}
    if glu:
        ref.update({"dgg": d["gg"].grad, "dbg": d["bgt"].grad, "dwg": d["wg"].grad})
    return f32, tl(conv).float(), stats, ref


@pytest.mark.parametrize("fill", [False, True], ids=["zeros", "filled"])
@pytest.mark.parametrize("B,T4,Cin,Cout,glu", [(3, 12, 256, 512, True), (5, 8, 512, 256, False), (1, 16, 256, 512, True)])
def test_trunk_layer_backward(mode, B, T4, Cin, Cout, glu, fill):
    """dx, the norm parameters' gradients and the weight gradients accumulate, dconv is stored.  The data gradient is K-split (16 slices of
    the 3072 | 768-long sum): in fixed mode the slices must reach dx in a fixed order (this test found them added with atomics there)."""
    L = lib()
    KW = 3
    f32, conv, stats, ref = _trunk_bwd_data(B, T4, Cin, Cout, glu)
    Cx = conv.shape[0]
    tl = lambda t: t.permute(1, 0, 2).contiguous().cuda()          # noqa: E731
    dy_d, conv_d, x_d, stats_d = tl(f32["dy"]), conv.cuda(), tl(f32["x"]), stats.cuda()
    dev = {k: f32[k].cuda() for k in ("w", "wg", "ga", "be", "gg", "bgt")}
    acc = [k for k in ("dx", "dga", "dbe", "dgg", "dbg", "dw", "dwg") if k in ref]
    pres = {k: _prefill(ref[k], fill, 150 + i) for i, k in enumerate(acc)}

    def fn():
        o = {k: _dev(pres[k]) for k in acc}
        o["dconv"] = _nan(Cx, B, T4)                                # a plain store
        wpack = torch.zeros(Cin * Cx * KW, device="cuda")
        check(L.mcvc_trunk_layer_backward(ptr(dy_d), ptr(conv_d), ptr(stats_d), ptr(dev["ga"]), ptr(dev["be"]),
                                          ptr(dev["gg"]) if glu else None, ptr(dev["bgt"]) if glu else None,
                                          ptr(dev["w"]), ptr(dev["wg"]) if glu else None, ptr(x_d), ptr(o["dx"]), ptr(o["dconv"]), ptr(o["dga"]),
                                          ptr(o["dbe"]), ptr(o.get("dgg")), ptr(o.get("dbg")), ptr(o["dw"]), ptr(o.get("dwg")), ptr(wpack),
                                          B, Cin, T4, Cout, KW, stream()), "trunk_layer_backward")
        return o
    out = _run(mode, fn)
    tag = "B%d-T%d-%s-%s" % (B, T4, "glu" if glu else "plain", "filled" if fill else "zeros")
    _gate("trunk_bwd", mode, tag + "-dconv", out["dconv"], None, ref["dconv"], 5e-5)
    for k in acc:
        _gate("trunk_bwd", mode, "%s-%s" % (tag, k), out[k], pres[k], ref[k], 5e-5)


# ---------------------------------------------------------------------------------------------------------------------------------------
# losses, the masked input and its gradient, axpy, the loss combiner, the vector activations
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_l1_and_lsgan_losses_accumulate(mode):
    L = lib()
    g = torch.Generator().manual_seed(17)
    a, b = torch.randn(3, 80, 64, generator=g), torch.randn(3, 80, 64, generator=g)
    ad, bd = a.cuda(), b.cuda()
    n = a.numel()
    l1 = float((a.double() - b.double()).abs().mean())
    gref = 10.0 * torch.sign(a.double() - b.double()) / n
    pre = _prefill(gref, True, 160)
    z = torch.randn(2, 1, 10, 8, generator=g)
    dd = torch.sigmoid(z).cuda()
    dz = dd.double().cpu()
    s0 = torch.tensor([0.75, -1.25, 2.5, 0.5])

    def fn():
        slots = s0.cuda()
        ga, gs = _dev(pre), _nan(*a.shape)
        check(L.mcvc_l1_loss(ptr(ad), ptr(bd), n, 10.0, ptr(slots[0:1]), ptr(slots[1:2]), ptr(ga), 1, stream()), "l1_loss +=")
        check(L.mcvc_l1_loss(ptr(ad), ptr(bd), n, 10.0, ptr(slots[0:1]), ptr(slots[1:2]), ptr(gs), 0, stream()), "l1_loss =")
        gl = _nan(*z.shape)
        check(L.mcvc_lsgan_loss(ptr(dd), z.numel(), 1.0, 0.5, ptr(slots[2:3]), ptr(slots[3:4]), ptr(gl), stream()), "lsgan_loss")
        return {"slots": slots, "ga": ga, "gs": gs, "gl": gl}
    out = _run(mode, fn)
    s = out["slots"].double().cpu()
    ls = float(((1.0 - dz) ** 2).mean())
    want = [0.75 + 2 * 10.0 * l1, -1.25 + 2 * l1, 2.5 + 0.5 * ls, 0.5 + ls]         # (two L1 calls on the same slots)
    for i in range(4):
        assert abs(float(s[i]) - want[i]) < 2e-6 * max(1.0, abs(want[i])), (i, float(s[i]), want[i])
    _gate("loss", mode, "l1-grad-accumulated", out["ga"], pre, gref, 1e-6)
    _gate("loss", mode, "l1-grad-stored", out["gs"], None, gref, 1e-6)
    _gate("loss", mode, "lsgan-grad", out["gl"], None, 0.5 * 2.0 * (dz - 1.0) / z.numel() * dz * (1.0 - dz), 1e-5)


@pytest.mark.parametrize("P", [80 * 20, 35])
def test_fif_input_and_its_gradient(mode, P):
    L = lib()
    N = 2
    g = torch.Generator().manual_seed(19)
    x = torch.randn(N, P, generator=g)
    mask = (torch.rand(N, P, generator=g) > 0.3).float()
    dxin = torch.randn(N, 2, P, generator=g)
    pre = torch.randn(N, P, generator=g)
    xd, md, dd = x.cuda(), mask.cuda(), dxin.cuda()

    def fn():
        xin, ds, da = _nan(N, 2, P), _nan(N, P), pre.cuda()
        check(L.mcvc_fif_input(ptr(xd), ptr(md), ptr(xin), N, P, stream()), "fif_input")
        check(L.mcvc_fif_input_grad(ptr(dd), ptr(md), ptr(ds), N, P, 0, stream()), "fif_input_grad =")
        check(L.mcvc_fif_input_grad(ptr(dd), ptr(md), ptr(da), N, P, 1, stream()), "fif_input_grad +=")
        return {"xin": xin, "ds": ds, "da": da}
    out = _run(mode, fn)
    assert torch.equal(out["xin"].cpu(), torch.stack((x * mask, mask), 1))
    assert torch.equal(out["ds"].cpu(), dxin[:, 0] * mask)
    assert torch.equal(out["da"].cpu(), pre + dxin[:, 0] * mask)          # one fp32 addition of the exact product: the same rounding


@pytest.mark.parametrize("offset", [0, 1])
def test_axpy(mode, offset):
    L = lib()
    n = 4 * 1003 + 3
    g = torch.Generator().manual_seed(23)
    x, y0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    alpha = 0.37

    def fn():
        y, xd = _dev(y0, offset), _dev(x, offset)
        check(L.mcvc_axpy(ptr(y), ptr(xd), alpha, n, stream()), "axpy")
        return {"y": y}
    out = _run(mode, fn)
    ref = y0.double() + float(np.float32(alpha)) * x.double()
    _gate("axpy", mode, "off%d" % offset, out["y"], None, ref, 1e-7)


def test_loss_combine_adds_in_index_order(mode):
    """Five pairs, repeated and skipped (-1) destinations; the weighted values go to slots 0 / 1, the plain means to slots 2 / 3, so the order
    within one pair does not matter and the order over k is the one of mcvc.h."""
    L = lib()
    g = torch.Generator().manual_seed(29)
    pairs = torch.randn(10, generator=g) * torch.tensor([1e3, 1.0, 1e-3, 1.0, 10.0, 1e-4, 1.0, 1e3, 0.1, 1.0])
    s0 = torch.randn(4, generator=g)
    loss_dst, term_dst = [0, 0, 1, -1, 0], [2, -1, 2, 3, 2]
    want = s0.clone()
    for k in range(5):
        if loss_dst[k] >= 0:
            want[loss_dst[k]] = want[loss_dst[k]] + pairs[2 * k]
        if term_dst[k] >= 0:
            want[term_dst[k]] = want[term_dst[k]] + pairs[2 * k + 1]
    ld, td = (ctypes.c_int * 5)(*loss_dst), (ctypes.c_int * 5)(*term_dst)
    pd = pairs.cuda()

    def fn():
        slots = s0.cuda()
        check(L.mcvc_loss_combine(ptr(pd), 5, ld, td, ptr(slots), stream()), "loss_combine")
        return {"slots": slots}
    out = _run(mode, fn)
    assert torch.equal(out["slots"].cpu(), want), (out["slots"].cpu(), want)


@pytest.mark.parametrize("H,W", [(8, 8), (5, 7)], ids=["vec-P64", "scalar-P35"])
@pytest.mark.parametrize("act", [ops.ACT_GLU, ops.ACT_SILU, ops.ACT_SIGMOID])
def test_activation_vector_and_scalar_kernels(mode, act, H, W):
    """P % 4 == 0 on aligned buffers: act_fwd_vec_kernel / act_bwd_vec_kernel; P = 35: the scalar kernels."""
    L = lib()
    g = torch.Generator().manual_seed(13)
    N, C, P = 2, 6, H * W
    x = torch.randn(N, 2 * C if act == ops.ACT_GLU else C, H, W, generator=g)
    xr = x.double().requires_grad_(True)
    if act == ops.ACT_GLU:
        ref = xr[:, :C] * torch.sigmoid(xr[:, C:])
    elif act == ops.ACT_SILU:
        ref = xr * torch.sigmoid(xr)
    else:
        ref = torch.sigmoid(xr)
    dy = torch.randn(ref.shape, generator=g)
    (rg,) = torch.autograd.grad(ref, xr, dy.double())

    def fn():
        xd, dyd = _dev(x), _dev(dy)
        y, dx = _nan(N, C, H, W), _nan(*x.shape)
        assert (xd.data_ptr() | dyd.data_ptr() | y.data_ptr() | dx.data_ptr()) % 16 == 0
        check(L.mcvc_act_forward(ptr(xd), ptr(y), N, C, P, act, stream()), "act_forward")
        check(L.mcvc_act_backward(ptr(xd), ptr(dyd), ptr(dx), N, C, P, act, stream()), "act_backward")
        return {"y": y, "dx": dx}
    out = _run(mode, fn)
    _gate("act", mode, "a%d-P%d-y" % (act, P), out["y"], None, ref.detach(), 1e-6)
    _gate("act", mode, "a%d-P%d-dx" % (act, P), out["dx"], None, rg, 1e-6)


# ---------------------------------------------------------------------------------------------------------------------------------------
# whole networks: a second backward pass into the same gradient tables, accumulate_dx = 1
# ---------------------------------------------------------------------------------------------------------------------------------------
def _twice_equals_double(single, double, what):
    for i, (a, b) in enumerate(zip(single, double)):
        if a is None:
            continue
        na = float(a.double().norm())
        if na < 1e-6:                                  # (conv biases in front of an InstanceNorm: mathematically zero)
            continue
        e = float((b.double() - 2.0 * a.double()).norm()) / (2.0 * na)
        assert e < 2e-5, (what, i, e)


def test_generator_backward_accumulates_gradients_and_dx(mode):
    L = lib()
    B, T = 1, 24
    gen = Generator()
    gen.load_state_dict(orc.filler_params("G", 37), strict=True)
    gen = gen.cuda()
    ps = list(gen.parameters())
    packed = gen.packed_weights(ps, force=True)
    n_scr = L.mcvc_gen_scratch_floats(B, T)
    stash, scratch = torch.zeros(L.mcvc_gen_stash_floats(B, T), device="cuda"), torch.zeros(n_scr, device="cuda")
    rng = torch.Generator().manual_seed(31)
    x, dout = torch.randn(B, 80, T, generator=rng).cuda(), torch.randn(B, 80, L.mcvc_gen_out_frames(T), generator=rng).cuda()
    m = torch.ones(B, 80, T)
    m[:, :, 5:11] = 0
    m = m.cuda()
    out = torch.empty(B, 80, L.mcvc_gen_out_frames(T), device="cuda")
    tab = ptr_table(ps)
    check(L.mcvc_gen_forward(tab, ptr(packed), ptr(x), ptr(m), ptr(out), ptr(stash), ptr(scratch), n_scr, B, T, stream()), "gen_forward")

    def backward(times):
        grads, dx = [torch.zeros_like(p) for p in ps], _nan(B, 80, T)
        for k in range(times):
            check(L.mcvc_gen_backward(tab, ptr(packed), ptr_table(grads), ptr(m), ptr(dout), ptr(dx), 1 if k else 0, ptr(stash), ptr(scratch), n_scr,
                                      B, T, stream(), None), "gen_backward")
        torch.cuda.synchronize()
        return grads + [dx]
    single, double = backward(1), backward(2)
    assert float(single[-1].norm()) > 0 and sum(float(t.norm()) > 1e-6 for t in single) > 40
    _twice_equals_double(single, double, "generator " + mode)


def test_discriminator_backward_accumulates_gradients_and_dx(mode):
    L = lib()
    B, T = 1, 24
    d = Discriminator()
    d.load_state_dict(orc.filler_params("D", 41), strict=True)
    d = d.cuda()
    ps = list(d.parameters())
    packed = d.packed_weights(ps)
    n_scr = L.mcvc_disc_scratch_floats(B, T)
    stash, scratch = torch.zeros(L.mcvc_disc_stash_floats(B, T), device="cuda"), torch.zeros(n_scr, device="cuda")
    rng = torch.Generator().manual_seed(43)
    x = torch.randn(B, 80, T, generator=rng).cuda()
    oshape = (B, 1, 10, L.mcvc_disc_out_frames(T))
    dout = torch.randn(oshape, generator=rng).cuda()
    out = torch.empty(oshape, device="cuda")
    tab = ptr_table(ps)
    check(L.mcvc_disc_forward(tab, ptr(packed), ptr(x), ptr(out), ptr(stash), ptr(scratch), n_scr, B, T, stream()), "disc_forward")

    def backward(times):
        grads = [None if 14 <= i <= 17 else torch.zeros_like(p) for i, p in enumerate(ps)]      # (downSample4 takes no part in forward)
        dx = _nan(B, 80, T)
        for k in range(times):
            check(L.mcvc_disc_backward(tab, ptr(packed), ptr_table(grads), ptr(dout), 0, ptr(dx), 1 if k else 0, ptr(stash), ptr(scratch), n_scr,
                                       B, T, stream(), None), "disc_backward")
        torch.cuda.synchronize()
        return grads + [dx]
    single, double = backward(1), backward(2)
    assert float(single[-1].norm()) > 0 and sum(t is not None and float(t.norm()) > 1e-6 for t in single) >= 8
    _twice_equals_double(single, double, "discriminator " + mode)


# ---------------------------------------------------------------------------------------------------------------------------------------
# ill-conditioned InstanceNorm inputs: a per-channel DC offset of 32 standard deviations.  Gate = twice the distance of the plain fp32
# PyTorch pipeline from the fp64 one, floored at the op's gate for well-conditioned inputs (the convention of tests/test_hip_audio.py).
# ---------------------------------------------------------------------------------------------------------------------------------------
OFFSET = 32.0


def _offset_gate(family, what, got, ref64, ref32, floor):
    d_ref = rel_l2(ref32, ref64)
    d_got = rel_l2(got, ref64)
    gate = max(2.0 * d_ref, floor)
    print("MODES %s offset32 %s kernel %.3e reference %.3e gate %.3e" % (family, what, d_got, d_ref, gate))
    assert d_got < gate, (family, what, d_got, d_ref, gate)


@pytest.mark.parametrize("N,C,H,W,act", [(2, 7, 3, 5, ops.ACT_GLU), (2, 128, 20, 16, ops.ACT_SILU)])
def test_instnorm_act_with_a_dc_offset_of_32_sigma(N, C, H, W, act):
    L = lib()
    inputs = _norm_inputs(N, C, H, W, act, False, OFFSET)
    y64, g64 = _norm_pipeline(inputs, act, C, torch.float64)
    y32, g32 = _norm_pipeline(inputs, act, C, torch.float32)
    pres = [torch.zeros(r.shape) for r in g64[1:]]
    out = _norm_launch(L, inputs, N, C, H, W, act, pres)
    torch.cuda.synchronize()
    tag = "%dx%dx%dx%d-a%d" % (N, C, H, W, act)
    _offset_gate("norm_fwd", tag + "-y", out["y"], y64, y32, 5e-5)
    _offset_gate("norm_bwd", tag + "-dx", out["dx"], g64[0], g32[0], 2e-4)
    for i in range(len(pres)):
        _offset_gate("norm_bwd", "%s-dp%d" % (tag, i), out["dp%d" % i], g64[i + 1], g32[i + 1], 2e-4)


def _offset_conv1d_operands(B, Cin, C, T, KW, gated, seed):
    """x with +-32 on every input channel; weights whose signed row sum is zero per tap except +-1 / Cin on the centre tap, so that the
    conv output of channel co is (unit-variance noise) +- 32: the offset reaches the normalisation, also next to the zero padding."""
    g = torch.Generator().manual_seed(seed)
    s = (torch.randint(0, 2, (Cin,), generator=g) * 2 - 1).float()
    x = torch.randn(B, Cin, T, generator=g) + OFFSET * s.view(1, Cin, 1)

    def mk():
        w = torch.randn(C, Cin, KW, generator=g) / (Cin * KW) ** 0.5
        w = w - (w * s.view(1, Cin, 1)).sum(1, keepdim=True) * s.view(1, Cin, 1) / Cin
        so = (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
        w[:, :, KW // 2] += so.view(C, 1) * s.view(1, Cin) / Cin
        return w
    w, wg = mk(), (mk() if gated else None)
    ga, be = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    gg, bg = (1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)) if gated else (None, None)
    return x, w, wg, ga, be, gg, bg


def _conv1d_norm_pipeline(x, w, wg, ga, be, gg, bg, b, bgate, pad, dtype):
    t = lambda v: v.to(dtype) if v is not None else None          # noqa: E731
    c0 = F.conv1d(t(x), t(w), t(b), padding=pad)
    z = F.instance_norm(c0, weight=t(ga), bias=t(be), eps=1e-5)
    if wg is not None:
        c1 = F.conv1d(t(x), t(wg), t(bgate), padding=pad)
        z = z * torch.sigmoid(F.instance_norm(c1, weight=t(gg), bias=t(bg), eps=1e-5))
    return z, c0


def test_trunk_layer_forward_with_a_dc_offset_of_32_sigma():
    L = lib()
    B, T4, Cin, Cout, KW = 3, 16, 256, 512, 3
    x, w, wg, ga, be, gg, bg = _offset_conv1d_operands(B, Cin, Cout, T4, KW, True, 51)
    g = torch.Generator().manual_seed(52)
    b, bgate = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    y64, c64 = _conv1d_norm_pipeline(x, w, wg, ga, be, gg, bg, b, bgate, 1, torch.float64)
    y32, _ = _conv1d_norm_pipeline(x, w, wg, ga, be, gg, bg, b, bgate, 1, torch.float32)
    ratio = float((c64.mean(2).abs() / c64.std(2)).median())
    assert ratio > 16.0, ratio                                  # the conv output really carries the offset
    dev = [t.cuda() for t in (w, b, ga, be, wg, bgate, gg, bg)]
    xt = x.permute(1, 0, 2).contiguous().cuda()
    conv_out, stats, y = _nan(2 * Cout, B, T4), _nan(B, 2 * Cout, 2), _nan(Cout, B, T4)
    check(L.mcvc_trunk_layer_forward(ptr(xt), *[ptr(t) for t in dev], None, ptr(conv_out), ptr(stats), ptr(y), B, Cin, T4, Cout, KW, stream()),
          "trunk_layer_forward")
    torch.cuda.synchronize()
    _offset_gate("trunk_fwd", "B3-T16-glu-y", y.permute(1, 0, 2), y64, y32, 5e-5)


def _bf16_round(t):
    return t.to(torch.bfloat16).float()


def test_bf16_trunk_layer_with_a_dc_offset_of_32_sigma():
    L = lib()
    B, W, Cin, C = 3, 16, 256, 512
    x, w, wg, ga, be, gg, bg = _offset_conv1d_operands(B, Cin, C, W, 3, True, 53)
    xb, wb, wgb = _bf16_round(x), _bf16_round(w), _bf16_round(wg)           # the operands the kernel multiplies
    y64, c64 = _conv1d_norm_pipeline(xb, wb, wgb, ga, be, gg, bg, None, None, 1, torch.float64)
    y32, _ = _conv1d_norm_pipeline(xb, wb, wgb, ga, be, gg, bg, None, None, 1, torch.float32)
    assert float((c64.mean(2).abs() / c64.std(2)).median()) > 16.0
    xd = x.cuda().to(torch.bfloat16).permute(0, 2, 1).contiguous()
    dev = [t.cuda() for t in (w, wg, ga, be, gg, bg)]
    y = torch.full((B, W, C), NAN, dtype=torch.bfloat16, device="cuda")
    wpack = torch.zeros(L.mcvc_bf16_trunk_layer_pack_bytes(Cin, C, 1), dtype=torch.uint8, device="cuda")
    check(L.mcvc_bf16_trunk_layer(ptr(xd), *[ptr(t) for t in dev], None, ptr(y), ptr(wpack), B, W, Cin, C, stream()), "bf16_trunk_layer")
    torch.cuda.synchronize()
    got = y.float().permute(0, 2, 1).cpu()
    assert torch.isfinite(got).all()
    _offset_gate("bf16_trunk_layer", "B3-W16-gated", got, _bf16_round(y64), _bf16_round(y32), 4e-3)


def test_bf16_conv2dto1d_norm_with_a_dc_offset_of_32_sigma():
    L = lib()
    B, W = 3, 16
    x, w, _, ga, be, _, _ = _offset_conv1d_operands(B, 5120, 256, W, 1, False, 55)          # the reference's channel order c * 20 + h
    xb, wb = _bf16_round(x), _bf16_round(w)
    y64, c64 = _conv1d_norm_pipeline(xb, wb, None, ga, be, None, None, None, None, 0, torch.float64)
    y32, _ = _conv1d_norm_pipeline(xb, wb, None, ga, be, None, None, None, None, 0, torch.float32)
    assert float((c64.mean(2).abs() / c64.std(2)).median()) > 16.0
    xm = x.cuda().to(torch.bfloat16).view(B, 256, 20, W).permute(0, 3, 2, 1).contiguous().view(B, W, 5120)       # [b][w][h * 256 + c]
    wd, gad, bed = w[:, :, 0].contiguous().cuda(), ga.cuda(), be.cuda()
    y = torch.full((B, W, 256), NAN, dtype=torch.bfloat16, device="cuda")
    wpack = torch.zeros(L.mcvc_bf16_c2d1d_pack_bytes(), dtype=torch.uint8, device="cuda")
    check(L.mcvc_bf16_c2d1d_norm(ptr(xm), ptr(wd), ptr(gad), ptr(bed), ptr(y), ptr(wpack), B, W, stream()), "bf16_c2d1d_norm")
    torch.cuda.synchronize()
    got = y.float().permute(0, 2, 1).cpu()
    assert torch.isfinite(got).all()
    _offset_gate("bf16_c2d1d_norm", "B3-W16", got, _bf16_round(y64), _bf16_round(y32), 4e-3)
