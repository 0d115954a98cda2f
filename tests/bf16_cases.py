"""The op-level cases of the bf16 convolution and InstanceNorm (tests/test_hip_bf16.py runs them on the GPU) with the kernel form each
convolution case must reach, their fp64 references, and the host-side view of the launcher's plan (mcvc_bf16_conv_plan, mcvc_gen_bf16_conv_plans: pure host code).  Shared with
tests/test_host_bf16_plan.py, which asserts on the CPU that every form the generator's forward reaches is reached by a case here.

Shape = (N, H, W, Cin, Cout, KH, KW, stride, pad_h, pad_w); plan key = (cfg, KWT, PPT, TH, TW, XCD block map): tile configuration
(0 = 128 x 128, 1 = 64 x 64, 2 = 32 x 128, 4 = 128 x 256, 5 = 128 x 512 channels x pixels), the instantiated compile-time kernel
width and input-prefetch depth of bf16_conv_kernel (0 = run-time width / synchronous staging), the pixel tile, and whether workgroups
map to tiles XCD-wise.

The large cases all have Cin = 64 (two channel chunks: the register prefetch "one chunk ahead" runs), N >= 2 and tiles that overhang
the image in both directions.  conv_config's thresholds put configuration 0 at >= 8.4 M outputs, the stride-2 configuration 4 at
>= 16.8 M and configuration 5 at >= 33.5 M, so these are the smallest shapes at which the forms exist (<= 53 GMAC each)."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

PLAN_FIELDS = ("cfg", "BM", "BN", "KWT", "PPT", "TH", "TW", "tiles_h", "tiles_w", "PH", "PW", "lds", "xcd")
ROW = 1 + len(PLAN_FIELDS)
# layer ids of the forward's plan rows (include/mcvc.h: 0 conv1, 1 downSample1, 2 downSample2, 3 conv2dto1d, 4 conv1dto2d, 5 upSample1,
# 6 upSample2, 7 last conv, 10 + i / 20 + i the residual blocks) -> stride as the forward runs the layer (csrc/infer_bf16.hip build_net:
# conv2dto1d is a 1 x 5 stride-5 convolution, the residual blocks' convolutions 1 x 6 with stride 2)
LAYER_STRIDE = {0: 1, 1: 2, 2: 2, 3: 5, 4: 1, 5: 1, 6: 1, 7: 1, **{10 + i: 2 for i in range(6)}, **{20 + i: 2 for i in range(6)}}

CONV_CASES = [
    # shape                                        plan key                      what it is in the generator
    ((2, 80, 64, 32, 256, 5, 1, 1, 2, 0),         (1, 1,  4,  8,   8, 1)),    # conv1 after the kw fold
    ((2, 80, 64, 128, 512, 5, 5, 2, 2, 2),        (1, 5, 12,  8,   8, 1)),    # downSample1 (value | gate)
    ((1, 40, 32, 256, 512, 5, 5, 2, 2, 2),        (1, 5, 12,  4,  16, 1)),    # downSample2
    ((2, 1, 16, 5120, 256, 1, 1, 1, 0, 0),        (1, 1,  4,  4,  16, 1)),    # conv2dto1d
    ((3, 1, 16, 256, 1024, 1, 3, 1, 0, 1),        (1, 3,  4,  1,  64, 0)),    # residual value | gate
    ((3, 1, 16, 512, 256, 1, 3, 1, 0, 1),         (1, 3,  4,  1,  64, 0)),    # residual out
    ((2, 1, 16, 256, 5120, 1, 1, 1, 0, 0),        (1, 1,  4,  4,  16, 0)),    # conv1dto2d
    ((1, 20, 16, 256, 1024, 5, 5, 1, 2, 2),       (1, 5,  4,  4,  16, 0)),    # upSample1
    ((1, 40, 32, 256, 512, 5, 5, 1, 2, 2),        (1, 5, 12,  8,   8, 1)),    # upSample2
    ((1, 80, 64, 128, 32, 5, 1, 1, 2, 0),         (2, 1,  4, 16,   8, 1)),    # last conv after the kw -> channel fold (32-row tile config)
    ((1, 13, 37, 64, 36, 3, 3, 1, 1, 1),          (1, 3,  4,  8,   8, 0)),    # ragged: overhanging tiles, Cout not a multiple of 32
    ((1, 21, 45, 32, 128, 5, 5, 2, 2, 2),         (1, 5, 12,  8,   8, 0)),    # ragged stride 2
    ((2, 1, 80, 1024, 256, 1, 5, 5, 0, 0),        (1, 5, 12,  1,  64, 1)),    # conv2dto1d as the forward runs it since r5: 1 x 5, stride 5 over [5 * W4 positions][1024 channels]
    ((3, 1, 32, 128, 1024, 1, 6, 2, 0, 2),        (1, 6,  4,  1,  64, 0)),    # residual value | gate as the forward runs it: 1 x 6, stride 2, two channel groups as positions
    ((3, 1, 32, 256, 256, 1, 6, 2, 0, 2),         (1, 6,  4,  1,  64, 0)),    # residual out, the same fold
    ((1, 9, 31, 32, 64, 3, 3, 3, 1, 1),           (1, 3, 12,  4,  16, 0)),    # a stride the generator does not use (general stride in the pixel addressing), ragged
    # ---- the forms of the large tiles
    ((3, 19, 566, 64, 1024, 5, 5, 1, 2, 2),       (5, 5, 17,  4, 128, 1)),    # upSample1 at 16 x 512 frames
    ((2, 38, 425, 64, 1024, 5, 5, 1, 2, 2),       (5, 5, 13,  8,  64, 1)),    # upSample2 at 16 x 512
    ((3, 37, 566, 64, 1024, 5, 5, 2, 2, 2),       (4, 5, 20,  8,  32, 1)),    # downSample1, downSample2 at 16 x 512
    ((2, 1, 8200, 64, 512, 1, 1, 1, 0, 0),        (0, 1,  4,  1, 128, 1)),    # conv1dto2d at 16 x 512
    ((2, 19, 428, 64, 512, 5, 5, 1, 2, 2),        (0, 5, 12,  4,  32, 1)),    # upSample1 at 8 x 256
    ((3, 38, 143, 64, 512, 5, 5, 1, 2, 2),        (0, 5, 12,  8,  16, 0)),    # upSample2 at 8 x 256; block map b % n_co
    ((2, 37, 425, 64, 1024, 5, 5, 2, 2, 2),       (0, 5, 12,  4,  32, 1)),    # downSample2 at 4 x 1001
    ((3, 77, 278, 64, 512, 5, 5, 2, 2, 2),        (0, 5, 12,  8,  16, 0)),    # downSample1 at 1 x 1601
    ((3, 77, 140, 64, 1024, 5, 5, 1, 2, 2),       (5, 5, 12, 16,  32, 1)),    # compiled; reachable at other aspect ratios
    ((2, 81, 200, 64, 1024, 5, 5, 1, 2, 2),       (5, 5,  0, 32,  16, 1)),    # 128 x 512 with the synchronous staging loop (upSample1 at 16 x 513)
    ((2, 38, 425, 64, 1024, 3, 3, 1, 1, 1),       (5, 3, 12,  8,  64, 1)),    # the 3-wide instantiations
    ((3, 19, 566, 64, 1024, 3, 3, 1, 1, 1),       (5, 3,  0,  4, 128, 1)),
    ((2, 19, 428, 64, 512, 3, 3, 1, 1, 1),        (0, 3,  4,  4,  32, 1)),
    ((2, 37, 425, 64, 1024, 3, 3, 2, 1, 1),       (0, 3, 12,  4,  32, 1)),
    ((2, 81, 50, 64, 1024, 5, 1, 1, 2, 0),        (0, 0,  0,  2,  64, 1)),    # run-time kernel width at BM = 128
    ((2, 1, 8080, 128, 1024, 1, 6, 2, 0, 2),      (1, 6,  4,  1,  64, 0)),    # residual value | gate, unfused trunk, B * W4 > 8064: was rejected (1001) on 128-row tiles
    ((3, 41, 179, 64, 384, 5, 5, 1, 2, 2),        (0, 5, 12,  2,  64, 0)),    # block map with three channel tiles (b % n_co)
    ((13, 80, 65, 64, 1024, 5, 5, 2, 2, 2),       (4, 5, 20, 16,  16, 1)),    # downSample1's tile at 32 x 65 frames: 16 x 16 stride 2, LDS full; was rejected (1001) by the pitch widening
    ((2, 1, 82000, 64, 256, 1, 5, 5, 0, 0),       (0, 5, 12,  1, 128, 0)),    # conv2dto1d (1 x 5, stride 5) on 128-row tiles: the unfused forward at 32 x 4096 frames
]


def conv_plan(L, shape):
    """(return code of the launch, {field: value}) for one mcvc_bf16_conv2d problem."""
    out = np.zeros(len(PLAN_FIELDS), dtype=np.int32)
    rc = L.mcvc_bf16_conv_plan(*shape, out.ctypes.data, out.size)
    return rc, dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def plan_key(p):
    return (p["cfg"], p["KWT"], p["PPT"], p["TH"], p["TW"], p["xcd"])


def forward_plans(L, B, T):
    """(return code, [(layer id, {field: value})]) of the generic convolutions of the bf16 forward at (B, T)."""
    n = ctypes.c_int(0)
    rows = np.zeros((64, ROW), dtype=np.int32)
    rc = L.mcvc_gen_bf16_conv_plans(B, T, rows.ctypes.data, rows.shape[0], ctypes.byref(n))
    assert 0 <= n.value <= rows.shape[0]
    return rc, [(int(r[0]), dict(zip(PLAN_FIELDS, (int(v) for v in r[1:])))) for r in rows[:n.value]]


def stride_class(stride):
    return stride if stride in (1, 2) else "other"


# ---- convolution reference ----------------------------------------------------------------------------------------------------
def conv_inputs(shape):
    """x bf16 NCHW, w fp32 OIHW (the library rounds it to bf16), bias fp32 -- on the CPU, seeded."""
    N, H, W, Cin, Cout, KH, KW, stride, ph, pw = shape
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, Cin, H, W, generator=g).to(torch.bfloat16)
    w = torch.randn(Cout, Cin, KH, KW, generator=g) / (Cin * KH * KW) ** 0.5
    b = torch.randn(Cout, generator=g)
    return x, w, b


def conv_reference(shape, x, w, b):
    """(ref, A): F.conv2d in fp64 on the bf16-rounded x and w with the fp32 bias as double, and the magnitude
    A = conv(|x|, |w|) + |b| in fp32 (it only scales the accumulation term of the bound)."""
    stride, pad = shape[7], (shape[8], shape[9])
    wq = w.to(torch.bfloat16)
    ref = F.conv2d(x.double(), wq.double(), b.double(), stride, pad)
    A = F.conv2d(x.float().abs(), wq.float().abs(), b.abs(), stride, pad)
    return ref, A


def conv_bound(shape, ref, A):
    """Per-element bound of a correct kernel, derived (not measured):  2^-8 |ref| + 2 (K + 1) 2^-24 A.
    First term: the half-ulp of the one round-to-nearest-even bf16 store.  Second: the first-order bound (K + 1) u A of an fp32 sum of
    K exact products plus bias in any order (u = 2^-24; bf16 x bf16 products are exact in fp32), doubled because the MFMA's internal
    adds are not promised to round to nearest."""
    K = shape[3] * shape[5] * shape[6]
    return ref.abs() * 2.0 ** -8 + A.double() * (2.0 * (K + 1) * 2.0 ** -24)


# ---- InstanceNorm + activation ------------------------------------------------------------------------------------------------
NORM_CASES = [
    # N, H, W, Cx, act, shuffle, res
    (2, 40, 32, 512, 1, 0, False), (3, 1, 16, 1024, 1, 0, False), (3, 1, 16, 256, 0, 0, True),
    (2, 20, 16, 1024, 2, 1, False), (1, 40, 128, 512, 2, 1, False), (2, 1, 128, 5120, 0, 0, False),
    # the dispatch brackets of mcvc_bf16_norm_launch: one launch with 4 pixels per thread for P <= 128, with 8 for 128 < P <= 256,
    # else statistics / finalize / apply -- P = 129 and 240 (ragged in the 8-pixel kernel), 256 (its last size), 257 (first generic),
    # generic P that is no multiple of the 64-pixel split (660, 340 with PixelShuffle), one split of 42 pixels
    (2, 1, 129, 256, 0, 0, True), (1, 12, 20, 512, 1, 0, False), (2, 1, 256, 256, 0, 0, False), (1, 1, 257, 64, 0, 0, False),
    (2, 20, 33, 512, 1, 0, False), (1, 20, 17, 1024, 2, 1, False), (1, 6, 7, 32, 2, 1, False),
]


def norm_inputs(case):
    """x bf16 NCHW, value / gate affine parameters fp32, residual bf16 NHWC or None -- on the CPU, seeded."""
    N, H, W, Cx, act, shuffle, res = case
    g = torch.Generator().manual_seed(11)
    x = (1.5 * torch.randn(N, Cx, H, W, generator=g) + 0.7).to(torch.bfloat16)
    C = Cx // 4 if shuffle else (Cx // 2 if act == 1 else Cx)
    ga, be = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    gg, bg = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    OH, OW = (2 * H, 2 * W) if shuffle else (H, W)
    r = torch.randn(N, OH, OW, C, generator=g).to(torch.bfloat16) if res else None
    return x, ga, be, gg, bg, r


def norm_reference(case, x, ga, be, gg, bg, r):
    """act(InstanceNorm(x)) (+ residual) in fp64, NCHW."""
    N, H, W, Cx, act, shuffle, res = case
    C = ga.numel()
    xf, ga, be, gg, bg = x.double(), ga.double(), be.double(), gg.double(), bg.double()
    if shuffle:
        z = F.instance_norm(F.pixel_shuffle(xf, 2), weight=ga, bias=be, eps=1e-5)
    elif act == 1:
        z = F.instance_norm(xf[:, :C], weight=ga, bias=be, eps=1e-5)
        zg = F.instance_norm(xf[:, C:], weight=gg, bias=bg, eps=1e-5)
    else:
        z = F.instance_norm(xf, weight=ga, bias=be, eps=1e-5)
    ref = z * torch.sigmoid(zg) if act == 1 else (z * torch.sigmoid(z) if act == 2 else z)
    if res:
        ref = ref + r.double().permute(0, 3, 1, 2)
    return ref


def rel_per_channel(got, ref):
    """relative L2 per (sample, channel) of NCHW tensors, in fp64"""
    d = (got.double() - ref.double()).flatten(2).norm(dim=2)
    return d / ref.double().flatten(2).norm(dim=2)
