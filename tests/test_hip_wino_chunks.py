"""GPU: Winograd passes that run in several chunks of samples, and the planner's 16384-tile boundary.

A Winograd pass keeps at most kWinoMaxTiles = 16384 tiles in its V / M workspaces (csrc/net.hip); a batch with more tiles runs as several
chunks of samples (wino_chunk, wino_nbc; wino_pass and wino_wgrad_pass own the loop).  Every other test keeps every pass in one chunk.  Here
two layers -- the smallest that still take the batched Winograd GEMM for forward, data gradient and weight gradient -- run at N = 3 with
50 x 111 = 5550 ragged 2x2 tiles per sample: 16384 / 5550 = 2 samples per pass, so the chunks are 2 + 1 and the last chunk is shorter than
the first (NT and NTp change between launches into the same buffers; the weight gradient's tile-major zero rows [NT, NTp) are rewritten
after a larger chunk; the weight gradients add up over the chunks; the x / y chunk offsets go through the phase gather and the PixelShuffle
store).

The conventions are those of tests/test_hip_ops_modes.py: both settings of mcvc_set_deterministic (fixed mode runs twice, bit-equal), y and
dx start NaN-filled, dw starts from zeros and from noise of the increment's rms, the reference is F.conv2d / torch.nn.grad in float64 on the
CPU from the same fp32 inputs, the gate is 5e-5 relative L2 -- on the whole tensor AND on every sample on its own, so that one wrong sample
in the short chunk is not diluted by the others.

A layer whose Winograd form is declined falls through to the direct kernels without saying so, so every case also proves which path ran:
the library's launch trace must show exactly one batched Winograd GEMM launch ("wino_gemm") per chunk and operation -- 2 at N = 3, 1 at
N = 2 for the same layer.

Every measured distance is printed as a line `MODES <family> <mode> <what> <distance> <gate>`, every launch count as `MODES <family> <mode>
<what> launches <kind> <n>` (pytest -s shows them)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from mask_cyclegan_vc._hip import check, lib, ptr, stream  # noqa: E402
from test_hip_model import _launches  # noqa: E402
from test_hip_ops_modes import _dev, _gate, _nan, _prefill, _run, mode  # noqa: E402,F401  (mode: the fixture)

GATE = 5e-5
WINO_MAX_TILES = 16384          # kWinoMaxTiles of csrc/net.hip

# name -> (Cin, Cout, branches, KH, KW, stride, ph, pw, H, W, pixel_shuffle)
CHUNKED = {
    "f25": (128, 128, 1, 5, 5, 1, 2, 2, 99, 221, 1),          # F(2x2,5x5), stride 1, PixelShuffle store
    "f23-phase": (32, 64, 2, 5, 5, 2, 2, 2, 198, 442, 0),     # F(2x2,3x3) over the four input phases, value | gate; outputs 99 x 221
}
N_CHUNKED = 3
# the boundary layer: N = 1, 128 x 128 = 16384 tiles | 129 x 128 = 16512 tiles
BOUNDARY = {
    "t16384": (64, 128, 1, 5, 5, 1, 2, 2, 256, 256, 0),
    "t16512": (64, 128, 1, 5, 5, 1, 2, 2, 258, 256, 0),
    "t16384-c128": (128, 128, 1, 5, 5, 1, 2, 2, 256, 256, 0),          # (data gradient only: 128 product rows, the batched GEMM's shape)
    "t16512-c128": (128, 128, 1, 5, 5, 1, 2, 2, 258, 256, 0),
}
LAYERS = dict(CHUNKED, **BOUNDARY)


def _tiles(name):
    Cin, Cout, nbr, KH, KW, s, ph, pw, H, W, sh = LAYERS[name]
    OH, OW = (H + 2 * ph - KH) // s + 1, (W + 2 * pw - KW) // s + 1
    IH, IW = (H, W) if s == 1 else (OH, OW)          # the stride-1 convolution's image: the layer's own, or the phase planes
    return ((IH + 1) // 2) * ((IW + 1) // 2)


def test_the_shapes_are_the_ones_the_chunk_rule_splits():
    """5550 tiles per sample: two samples fit 16384 tiles, three do not; the boundary shapes sit at 16384 and one tile row above."""
    for name in CHUNKED:
        t = _tiles(name)
        assert t == 50 * 111 == 5550
        assert 2 * t <= WINO_MAX_TILES < 3 * t
    assert _tiles("t16384") == WINO_MAX_TILES and _tiles("t16512") == 16512


@functools.lru_cache(maxsize=None)
def _data(name, N):
    """fp32 operands (x, [w], [b], dy) of N samples.  The draws of sample n do not depend on N: N = 2 is the first two samples of N = 3."""
    Cin, Cout, nbr, KH, KW, s, ph, pw, H, W, sh = LAYERS[name]
    g = torch.Generator().manual_seed(61)
    ws = [torch.randn(Cout, Cin, KH, KW, generator=g) / np.sqrt(Cin * KH * KW) for _ in range(nbr)]
    bs = [torch.randn(Cout, generator=g) for _ in range(nbr)]
    OH, OW = (H + 2 * ph - KH) // s + 1, (W + 2 * pw - KW) // s + 1
    n_max = max(N, N_CHUNKED)
    x = torch.randn(n_max, Cin, H, W, generator=g)
    dy = torch.randn(n_max, nbr * Cout, OH, OW, generator=g)
    return x[:N].contiguous(), ws, bs, dy[:N].contiguous()


@functools.lru_cache(maxsize=None)
def _ref(name, N, what):
    """The float64 reference of one operation, computed once and shared (never written to).  "wgrad": one tensor per branch."""
    Cin, Cout, nbr, KH, KW, s, ph, pw, H, W, sh = LAYERS[name]
    x, ws, bs, dy = _data(name, N)
    wcat, bcat = torch.cat(ws, 0).double(), torch.cat(bs, 0).double()
    if what == "fwd":
        y = F.conv2d(x.double(), wcat, bcat, stride=s, padding=(ph, pw))
        return F.pixel_shuffle(y, 2) if sh else y
    if what == "dgrad":
        return torch.nn.grad.conv2d_input(x.shape, wcat, dy.double(), stride=s, padding=(ph, pw))
    dw = torch.nn.grad.conv2d_weight(x.double(), wcat.shape, dy.double(), stride=s, padding=(ph, pw))
    return tuple(dw[i * Cout:(i + 1) * Cout] for i in range(nbr))


class _Layer(object):
    """One layer's device operands and the three op-level launches, each into fresh destinations."""

    def __init__(self, name, N, scheme=1):
        self.L = lib()
        Cin, Cout, nbr, KH, KW, s, ph, pw, H, W, sh = LAYERS[name]
        self.name, self.N, self.nbr, self.sh, self.scheme = name, N, nbr, sh, scheme
        self.spec = (Cin, Cout, nbr, KH, KW, s, ph, pw)
        self.dims = (N, H, W)
        x, ws, bs, dy = _data(name, N)
        OH, OW = dy.shape[2], dy.shape[3]
        self.x_shape = tuple(x.shape)
        self.y_shape = (N, nbr * Cout // 4, 2 * OH, 2 * OW) if sh else tuple(dy.shape)
        self.n_scr = self.L.mcvc_layer_scratch_floats(N, H, W, *self.spec)
        assert self.n_scr > 0
        self.packed = torch.zeros(self.L.mcvc_layer_packed_floats(*self.spec), device="cuda")
        self.wd, bd = [w.cuda() for w in ws], [b.cuda() for b in bs]
        self.w1, b1 = (self.wd[1], bd[1]) if nbr == 2 else (None, None)
        check(self.L.mcvc_layer_pack(ptr(self.wd[0]), ptr(bd[0]), ptr(self.w1), ptr(b1), ptr(self.packed), *self.spec, stream()), "layer_pack")
        self.xd, self.dyd = x.cuda(), dy.cuda()
        self.scratch = None

    def fresh_scratch(self):
        self.scratch = None                      # (the op-level workspaces are sized for the whole batch: one at a time)
        self.scratch = torch.zeros(self.n_scr, device="cuda")

    def forward(self):
        y = _nan(*self.y_shape)
        rc = self.L.mcvc_layer_forward(ptr(self.xd), ptr(self.packed), ptr(self.wd[0]), ptr(self.w1), ptr(y), ptr(self.scratch), self.n_scr,
                                       *self.dims, *self.spec, self.scheme, self.sh, stream())
        return rc, y

    def dgrad(self):
        dx = _nan(*self.x_shape)
        rc = self.L.mcvc_layer_dgrad(ptr(self.dyd), ptr(self.packed), ptr(self.wd[0]), ptr(self.w1), ptr(dx), ptr(self.scratch), self.n_scr,
                                     *self.dims, *self.spec, self.scheme, stream())
        return rc, dx

    def wgrad(self, pres):
        dws = [_dev(p) for p in pres]
        rc = self.L.mcvc_layer_wgrad(ptr(self.xd), ptr(self.dyd), ptr(dws[0]), ptr(dws[1]) if self.nbr == 2 else None, ptr(self.scratch),
                                     self.n_scr, *self.dims, *self.spec, self.scheme, stream())
        return rc, dws

    def all_ops(self, pres):
        """fn of _run: fresh workspaces and destinations, the three launches, the results."""
        self.fresh_scratch()
        rc, y = self.forward()
        check(rc, "layer_forward")
        rc, dx = self.dgrad()
        check(rc, "layer_dgrad")
        rc, dws = self.wgrad(pres)
        check(rc, "layer_wgrad")
        out = {"y": y, "dx": dx}
        out.update({"dw%d" % i: d for i, d in enumerate(dws)})
        return out

    def launches(self, kinds, pres):
        """{op: {kind: launches}} of one more run of each operation, one trace per (operation, kind)."""
        self.fresh_scratch()
        ops = {"fwd": lambda: check(self.forward()[0], "layer_forward"), "dgrad": lambda: check(self.dgrad()[0], "layer_dgrad"),
               "wgrad": lambda: check(self.wgrad(pres)[0], "layer_wgrad")}
        return {op: {k: _launches(k, fn) for k in kinds} for op, fn in ops.items()}


def _gate_samples(family, mode, what, got, ref):
    """The gate on the whole tensor and on every sample on its own."""
    _gate(family, mode, what, got, None, ref, GATE)
    for n in range(ref.shape[0]):
        _gate(family, mode, "%s[%d]" % (what, n), got[n], None, ref[n], GATE)


def _check_counts(family, mode, tag, counts, kind, want):
    for op in ("fwd", "dgrad", "wgrad"):
        n = counts[op][kind]
        print("MODES %s %s %s-%s launches %s %d" % (family, mode, tag, op, kind, n))
    for op in ("fwd", "dgrad", "wgrad"):
        assert want is None or counts[op][kind] == want[op], (family, mode, tag, op, kind, counts[op][kind], want[op])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. three samples of 5550 tiles: chunks of 2 + 1
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [False, True], ids=["zeros", "filled"])
@pytest.mark.parametrize("name", sorted(CHUNKED))
def test_chunked_layer_ops(mode, name, fill):
    N = N_CHUNKED
    layer = _Layer(name, N)
    y_ref, dx_ref, dw_ref = _ref(name, N, "fwd"), _ref(name, N, "dgrad"), _ref(name, N, "wgrad")
    pres = [_prefill(r, fill, 170 + i) for i, r in enumerate(dw_ref)]
    out = _run(mode, lambda: layer.all_ops(pres))
    tag = "%s-N%d-%s" % (name, N, "filled" if fill else "zeros")
    _gate_samples("chunk_fwd", mode, tag, out["y"], y_ref)
    _gate_samples("chunk_dgrad", mode, tag, out["dx"], dx_ref)
    for i in range(layer.nbr):
        _gate("chunk_wgrad", mode, "%s-dw%d" % (tag, i), out["dw%d" % i], pres[i], dw_ref[i], GATE)
    counts = layer.launches(("wino_gemm",), pres)
    _check_counts("chunk", mode, tag, counts, "wino_gemm", {"fwd": 2, "dgrad": 2, "wgrad": 2})


@pytest.mark.parametrize("name", sorted(CHUNKED))
def test_two_samples_run_as_one_pass(name):
    """The same layers at N = 2 (11100 tiles): one Winograd GEMM launch per operation -- the count above is the chunk rule's, not the
    layer's.  y and dx are per sample: the first two samples of the N = 3 references."""
    layer = _Layer(name, 2)
    dw_shapes = [w.shape for w in layer.wd]
    pres = [torch.zeros(s) for s in dw_shapes]
    out = _run("atomic", lambda: layer.all_ops(pres))
    tag = "%s-N2" % name
    _gate_samples("chunk_fwd", "atomic", tag, out["y"], _ref(name, N_CHUNKED, "fwd")[:2])
    _gate_samples("chunk_dgrad", "atomic", tag, out["dx"], _ref(name, N_CHUNKED, "dgrad")[:2])
    counts = layer.launches(("wino_gemm",), pres)
    _check_counts("chunk", "atomic", tag, counts, "wino_gemm", {"fwd": 1, "dgrad": 1, "wgrad": 1})


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the planner's boundary: 16384 tiles in one sample still run Winograd, one tile row more declines it
#
# Which kernel multiplies is the planner's choice per operation (wino_pass): the batched Winograd GEMM takes products of M % 128 == 0 output
# rows.  The data gradient of the 64 -> 128 layer has M = Cin = 64 rows, so its 36 products run as ONE launch of the direct-convolution
# kernel over 36 images between the same two transform launches -- a Winograd pass without a "wino_gemm" launch.  For that operation the
# trace proves the path by the transforms (2 "elementwise" launches, none on the direct kernels), and the data gradient of a 128 -> 128
# layer at the same two image sizes carries the Winograd GEMM count.
# ---------------------------------------------------------------------------------------------------------------------------------------
def _boundary(name):
    layer = _Layer(name, 1)
    y_ref, dx_ref, dw_ref = _ref(name, 1, "fwd"), _ref(name, 1, "dgrad"), _ref(name, 1, "wgrad")
    pres = [torch.zeros(r.shape) for r in dw_ref]
    out = _run("atomic", lambda: layer.all_ops(pres))
    _gate_samples("boundary_fwd", "atomic", name, out["y"], y_ref)
    _gate_samples("boundary_dgrad", "atomic", name, out["dx"], dx_ref)
    _gate("boundary_wgrad", "atomic", name + "-dw0", out["dw0"], pres[0], dw_ref[0], GATE)
    return layer.launches(("wino_gemm", "elementwise"), pres)


def _boundary_dgrad_128(name):
    """The data gradient alone of the 128 -> 128 layer: gated, then traced."""
    layer = _Layer(name, 1)
    layer.fresh_scratch()
    rc, dx = layer.dgrad()
    check(rc, "layer_dgrad")
    torch.cuda.synchronize()
    _gate_samples("boundary_dgrad", "atomic", name, dx, _ref(name, 1, "dgrad"))
    n = _launches("wino_gemm", lambda: check(layer.dgrad()[0], "layer_dgrad"))
    print("MODES boundary atomic %s-dgrad launches wino_gemm %d" % (name, n))
    return n


def test_16384_tiles_in_one_sample_still_run_winograd():
    """H = W = 256: exactly kWinoMaxTiles tiles.  One Winograd GEMM launch per operation; the 64 -> 128 layer's data gradient (64 product
    rows) multiplies on the 36-image convolution launch between its two transforms instead."""
    counts = _boundary("t16384")
    _check_counts("boundary", "atomic", "t16384", counts, "elementwise", None)
    _check_counts("boundary", "atomic", "t16384", counts, "wino_gemm", {"fwd": 1, "dgrad": 0, "wgrad": 1})
    assert counts["dgrad"]["elementwise"] == 2, counts          # input transform + output transform: the Winograd pass ran
    assert _boundary_dgrad_128("t16384-c128") == 1


def test_16512_tiles_in_one_sample_decline_winograd():
    """H = 258, W = 256: 129 x 128 tiles.  No Winograd GEMM launch and no transform launch in forward and data gradient; the entries do not
    refuse the shape: the direct kernels' results pass the same gates."""
    counts = _boundary("t16512")
    _check_counts("boundary", "atomic", "t16512", counts, "elementwise", None)
    _check_counts("boundary", "atomic", "t16512", counts, "wino_gemm", {"fwd": 0, "dgrad": 0, "wgrad": 0})
    assert counts["fwd"]["elementwise"] == 0 and counts["dgrad"]["elementwise"] == 0, counts
    assert _boundary_dgrad_128("t16512-c128") == 0
