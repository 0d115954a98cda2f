"""GPU: the bf16 inference path (csrc/bf16_kernels.hip, infer_bf16.hip) -- BASELINE configs[4].

Single ops against a plain PyTorch fp32 reference evaluated on the SAME bf16-rounded operands (so the comparison measures the
kernel -- accumulation order and the one bf16 rounding of the output -- not the quantisation of the inputs): 4e-3 relative L2
(bf16 has 8 mantissa bits: output rounding alone is ~2.3e-3 rms); the generic convolution also element by element against fp64, in
every tile form the forward runs, and InstanceNorm per (sample, channel).  Whole generator against the CPU oracle in fp32: gate 2e-2
relative L2, at small shapes, ragged T, and the full bs=16 x 512 frames configuration."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import mcvc_oracle as orc  # noqa: E402
from mask_cyclegan_vc import _hip  # noqa: E402
from mask_cyclegan_vc._hip import check, lib, ptr, stream  # noqa: E402
from mask_cyclegan_vc.model import Generator  # noqa: E402
from bf16_cases import (CONV_CASES, NORM_CASES, conv_bound, conv_inputs, conv_plan, conv_reference, norm_inputs, norm_reference,  # noqa: E402
                        plan_key, rel_per_channel)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


CANARY = 0x7FA5                 # a bf16 NaN bit pattern (exponent all ones, mantissa 0x25): no finite convolution stores it
MARGIN = 1 << 19                # elements on either side of y: 1 MiB


@pytest.mark.parametrize("shape,key", CONV_CASES, ids=["-".join(map(str, s)) for s, _ in CONV_CASES])
def test_bf16_conv_matches_fp32_conv_on_the_same_rounded_operands(shape, key):
    """Every element of every case against F.conv2d in fp64 on the CPU, on the bf16-rounded x and w with the fp32 bias as double:

        |got - ref| <= 2^-8 |ref| + 2 (K + 1) 2^-24 A,     A = conv(|x|, |w|) + |b|,  K = Cin KH KW

    (bf16_cases.conv_bound: half an ulp of the kernel's one bf16 store plus the first-order bound of an fp32 sum of K exact products and
    the bias in any order, doubled for the MFMA's internal adds; derived, not tuned -- a torch fp32 conv rounded to bf16 peaks at 0.95
    of it, so one wrong tap, halo pixel or overhanging column fails).  No element is masked out or sampled; the 4e-3 whole-tensor
    relative L2 stays beside it.  y sits inside a larger buffer of a non-finite bit pattern with 1 MiB on either side: every element of y
    must have been overwritten and both margins must be bit-identical afterwards.  Each case first asserts, through the host-side plan,
    that it still reaches the kernel form it is there for (cfg, KWT, PPT, TH x TW, block map): tests/bf16_cases.py.

    Not reachable in the release build through any shape, and untested: configuration 4 at stride 1 (configuration 5 always wins when
    the layer is not gated), configuration 3 (experiments build only), and the fused-GLU epilogue of the generic kernel (conv1 has its
    own kernel: test_bf16_fused_conv1_matches_fp32_on_the_same_rounded_operands)."""
    L = lib()
    N, H, W, Cin, Cout, KH, KW, stride, ph, pw = shape
    rc, plan = conv_plan(L, shape)
    assert rc == 0 and plan_key(plan) == key, (rc, plan_key(plan), key)
    x, w, b = conv_inputs(shape)
    x_nhwc = x.cuda().permute(0, 2, 3, 1).contiguous()
    wd, bd = w.cuda(), b.cuda()
    OH, OW = (H + 2 * ph - KH) // stride + 1, (W + 2 * pw - KW) // stride + 1
    n_y = N * OH * OW * Cout
    buf = torch.full((MARGIN + n_y + MARGIN,), CANARY, dtype=torch.int16, device="cuda")
    y_bits = buf[MARGIN:MARGIN + n_y]
    y = y_bits.view(torch.bfloat16).view(N, OH, OW, Cout)
    wpack = torch.zeros(L.mcvc_bf16_conv2d_pack_bytes(Cout, Cin, KH, KW), dtype=torch.uint8, device="cuda")
    check(L.mcvc_bf16_conv2d(ptr(x_nhwc), ptr(wd), ptr(bd), ptr(y), ptr(wpack), N, H, W, Cin, Cout, KH, KW, stride, ph, pw, stream()), "bf16_conv2d")
    ref, A = conv_reference(shape, x, w, b)                  # (CPU, while the kernel runs)
    torch.cuda.synchronize()
    assert int((y_bits == CANARY).sum()) == 0, "elements of y the kernel never wrote"
    assert bool((buf[:MARGIN] == CANARY).all()) and bool((buf[MARGIN + n_y:] == CANARY).all()), "the kernel wrote outside y"
    ref, A = ref.cuda(), A.cuda()
    got = y.permute(0, 3, 1, 2).double()
    err, bound = (got - ref).abs(), conv_bound(shape, ref, A)
    ratio = float((err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
    e = float((got - ref).norm() / ref.norm())
    print("bf16 conv %s: plan (cfg %d, KWT %d, PPT %d, %d x %d, xcd %d)  worst |err| / bound %.3f  rel-L2 %.3e"
          % ((shape,) + key + (ratio, e)))
    bad = ~(err <= bound)
    assert not bool(bad.any()), (int(bad.sum()), ratio, [tuple(int(v) for v in i) for i in bad.nonzero()[:8]])
    assert e < 4e-3, e


@pytest.mark.parametrize("B,T,masked", [(2, 64, True), (1, 65, False), (3, 40, True), (1, 512, True), (2, 20, False)])
def test_bf16_fused_conv1_matches_fp32_on_the_same_rounded_operands(B, T, masked):
    """r6: conv1 + its input preparation + its gated GLU in ONE launch (bf16_conv1_fused_kernel: the (x * mask, mask) strip built in LDS from the
    fp32 inputs, the layer's weights in registers) -- model.py:241-242.  Reference: F.conv2d on the bf16-rounded stack(x * mask, mask) with
    the bf16-rounded weights, fp32 bias, value * sigmoid(gate); ragged T (strips of 32 columns overhang), T < 32, mask = None (ones)."""
    L = lib()
    g = torch.Generator().manual_seed(23)
    x = torch.randn(B, 80, T, generator=g).cuda()
    mask = None
    if masked:
        mask = torch.ones(B, 80, T)
        for b in range(B):
            s0 = int(torch.randint(0, max(T - 12, 1), (1,), generator=g)); mask[b, :, s0:s0 + min(12, T // 2)] = 0.0
        mask = mask.cuda()
    w = (torch.randn(128, 2, 5, 15, generator=g) / 150 ** 0.5).cuda(); wg = (torch.randn(128, 2, 5, 15, generator=g) / 150 ** 0.5).cuda()
    bv, bg = torch.randn(128, generator=g).cuda(), torch.randn(128, generator=g).cuda()
    y = torch.full((B, 80, T, 128), float("nan"), dtype=torch.bfloat16, device="cuda")
    wpack = torch.zeros(L.mcvc_bf16_conv1_glu_pack_bytes(), dtype=torch.uint8, device="cuda")
    check(L.mcvc_bf16_conv1_glu(ptr(x), ptr(mask), ptr(w), ptr(bv), ptr(wg), ptr(bg), ptr(y), ptr(wpack), B, T, stream()), "bf16_conv1_glu")
    m = mask if mask is not None else torch.ones_like(x)
    xin = torch.stack((x * m, m), dim=1).to(torch.bfloat16).float()
    v = F.conv2d(xin, w.to(torch.bfloat16).float(), bv, 1, (2, 7))
    gt = F.conv2d(xin, wg.to(torch.bfloat16).float(), bg, 1, (2, 7))
    ref = v * torch.sigmoid(gt)
    got = y.float().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    e = rel(got, ref)
    assert e < 4e-3, e


@pytest.mark.parametrize("B,W", [(3, 16), (16, 128), (1, 17), (9, 100), (2, 2)])
def test_bf16_fused_conv2dto1d_norm_matches_fp32_on_the_same_rounded_operands(B, W):
    """r6: conv2dto1d (5120 -> 256, k = 1) + its InstanceNorm in ONE launch (bf16_c2d1d_kernel: X through a four-stage LDS-DMA ring with swizzled
    16-byte pieces, operand-order weights in a register ring, hand-counted vmcnt waits) -- model.py:142-146, 249-255.  The kernel reads the
    layout the forward produces (memory channel h * 256 + c = reference channel c * 20 + h) and the weight in the reference's order.
    B = 9 / 16: more than one group of eight samples (the workgroup -> (sample, channel tile) map); ragged W; W = 2."""
    L = lib()
    g = torch.Generator().manual_seed(41)
    xr = torch.randn(B, 5120, W, generator=g).cuda().to(torch.bfloat16)               # the reference's channel order c * 20 + h
    w = (torch.randn(256, 5120, generator=g) / 5120 ** 0.5).cuda()
    ga, be = (1 + 0.2 * torch.randn(256, generator=g)).cuda(), (0.3 * torch.randn(256, generator=g)).cuda()
    xm = xr.view(B, 256, 20, W).permute(0, 3, 2, 1).contiguous().view(B, W, 5120)       # [b][w][h * 256 + c]
    y = torch.full((B, W, 256), float("nan"), dtype=torch.bfloat16, device="cuda")
    wpack = torch.zeros(L.mcvc_bf16_c2d1d_pack_bytes(), dtype=torch.uint8, device="cuda")
    check(L.mcvc_bf16_c2d1d_norm(ptr(xm), ptr(w), ptr(ga), ptr(be), ptr(y), ptr(wpack), B, W, stream()), "bf16_c2d1d_norm")
    z = F.instance_norm(F.conv1d(xr.float(), w.to(torch.bfloat16).float().unsqueeze(2)), weight=ga, bias=be, eps=1e-5)
    got = y.float().permute(0, 2, 1)
    assert torch.isfinite(got).all()
    assert rel(got, z) < 4e-3, rel(got, z)


@pytest.mark.parametrize("B,W,Cin,C,gated,res", [(3, 16, 256, 512, True, False), (3, 16, 512, 256, False, True), (2, 128, 256, 512, True, False),
                                                  (2, 128, 512, 256, False, True), (1, 17, 256, 512, True, False), (2, 100, 512, 256, False, False),
                                                  (1, 2, 256, 32, False, True), (2, 33, 512, 64, True, False)])
def test_bf16_fused_trunk_layer_matches_fp32_on_the_same_rounded_operands(B, W, Cin, C, gated, res):
    """r6: a residual-block layer (model.py:47-76) in ONE launch at inference -- conv1d(k = 3) + InstanceNorm1d + GLU / residual
    (bf16_trunk_layer_kernel: the sample's row block staged once in LDS, weights streamed in MFMA operand order, statistics on the fp32
    accumulators).  Reference: F.conv1d on the bf16-rounded x with bf16-rounded weights, F.instance_norm, fp32; W = 16 (64 frames), 128 (512
    frames: the benchmark shape), ragged widths, a single column."""
    L = lib()
    g = torch.Generator().manual_seed(31)
    x = torch.randn(B, Cin, W, generator=g).cuda().to(torch.bfloat16)
    w = (torch.randn(C, Cin, 3, generator=g) / (3 * Cin) ** 0.5).cuda()
    wg = (torch.randn(C, Cin, 3, generator=g) / (3 * Cin) ** 0.5).cuda() if gated else None
    ga, be = (1 + 0.2 * torch.randn(C, generator=g)).cuda(), (0.3 * torch.randn(C, generator=g)).cuda()
    gg, bg = ((1 + 0.2 * torch.randn(C, generator=g)).cuda(), (0.3 * torch.randn(C, generator=g)).cuda()) if gated else (None, None)
    r = torch.randn(B, W, C, generator=g).cuda().to(torch.bfloat16) if res else None
    y = torch.full((B, W, C), float("nan"), dtype=torch.bfloat16, device="cuda")
    wpack = torch.zeros(L.mcvc_bf16_trunk_layer_pack_bytes(Cin, C, 1 if gated else 0), dtype=torch.uint8, device="cuda")
    check(L.mcvc_bf16_trunk_layer(ptr(x.permute(0, 2, 1).contiguous()), ptr(w), ptr(wg), ptr(ga), ptr(be), ptr(gg), ptr(bg), ptr(r), ptr(y), ptr(wpack),
                                  B, W, Cin, C, stream()), "bf16_trunk_layer")
    xf = x.float()
    z = F.instance_norm(F.conv1d(xf, w.to(torch.bfloat16).float(), None, 1, 1), weight=ga, bias=be, eps=1e-5)
    if gated:
        z = z * torch.sigmoid(F.instance_norm(F.conv1d(xf, wg.to(torch.bfloat16).float(), None, 1, 1), weight=gg, bias=bg, eps=1e-5))
    if res:
        z = z + r.float().permute(0, 2, 1)
    got = y.float().permute(0, 2, 1)
    assert torch.isfinite(got).all()
    assert rel(got, z) < 4e-3, rel(got, z)


@pytest.mark.parametrize("B,T", [(2, 64), (1, 65), (1, 512), (3, 20), (1, 240)])
def test_bf16_fused_last_conv_matches_fp32_on_the_same_rounded_operands(B, T):
    """r6: the generator's last conv (128 -> 1, 5 x 15; model.py:207-211) in ONE launch (bf16_last_fused_kernel: 15 kernel columns as MFMA rows,
    weights in registers, every input row loaded once for its five output rows, fp32 kernel-column sum through LDS).  Reference: F.conv2d on
    the bf16 activations with bf16-rounded weights in fp32.  The output is fp32 (no output rounding): 1e-3.  T = 65 / 240 / 20: ragged strips
    of 114 output columns, a strip narrower than one tile."""
    L = lib()
    g = torch.Generator().manual_seed(29)
    x = torch.randn(B, 128, 80, T, generator=g).cuda().to(torch.bfloat16)
    w = (torch.randn(1, 128, 5, 15, generator=g) / (128 * 75) ** 0.5).cuda()
    b = torch.randn(1, generator=g).cuda()
    out = torch.full((B, 80, T), float("nan"), device="cuda")
    wpack = torch.zeros(L.mcvc_bf16_last_conv_pack_bytes(), dtype=torch.uint8, device="cuda")
    check(L.mcvc_bf16_last_conv(ptr(x.permute(0, 2, 3, 1).contiguous()), ptr(w), ptr(b), ptr(out), ptr(wpack), B, T, stream()), "bf16_last_conv")
    ref = F.conv2d(x.float(), w.to(torch.bfloat16).float(), b, 1, (2, 7))[:, 0]
    assert torch.isfinite(out).all()
    e = rel(out, ref)
    assert e < 1e-3, e


@pytest.mark.parametrize("N,H,W,Cx,act,shuffle,res", NORM_CASES)
def test_bf16_instnorm_act_matches_fp32(N, H, W, Cx, act, shuffle, res):
    """Against act(InstanceNorm(x)) in fp64 on the CPU: 4e-3 relative L2 on the whole tensor AND per (sample, output channel) -- one channel
    with wrong statistics is invisible in the whole-tensor figure (tests/test_host_bf16_plan.py checks on the CPU that output rounding alone
    stays under the bar for every channel of every case).  y starts as NaN and must come back finite.  The cases cover the launcher's
    three brackets -- one launch with 4 / 8 pixels per thread (P <= 128 / <= 256), else statistics, finalize, apply: bf16_cases.NORM_CASES."""
    L = lib()
    case = (N, H, W, Cx, act, shuffle, res)
    x, ga, be, gg, bg, r = norm_inputs(case)
    ref = norm_reference(case, x, ga, be, gg, bg, r)
    C = ga.numel()
    OH, OW = (2 * H, 2 * W) if shuffle else (H, W)
    xd, rd = x.cuda(), (r.cuda() if res else None)
    gad, bed, ggd, bgd = ga.cuda(), be.cuda(), gg.cuda(), bg.cuda()
    y = torch.full((N, OH, OW, C), float("nan"), dtype=torch.bfloat16, device="cuda")
    scratch = torch.zeros(N * 65 * Cx * 2, device="cuda")
    check(L.mcvc_bf16_instnorm_act(ptr(xd.permute(0, 2, 3, 1).contiguous()), ptr(gad), ptr(bed), ptr(ggd), ptr(bgd), ptr(rd), ptr(y), ptr(scratch),
                                   N, H, W, Cx, act, 1 if shuffle else 0, stream()), "bf16_instnorm_act")
    got = y.cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(got.float()).all()
    e = rel(got, ref)
    pc = rel_per_channel(got, ref)
    print("bf16 instnorm %r: rel-L2 %.3e, worst (sample, channel) %.3e" % (case, e, float(pc.max())))
    assert e < 4e-3, e
    assert float(pc.max()) < 4e-3, (float(pc.max()), [tuple(int(v) for v in i) for i in (pc >= 4e-3).nonzero()[:8]])


def _gen(seed):
    g = Generator()
    p = orc.filler_params("G", seed)
    g.load_state_dict(p, strict=True)
    return g.cuda(), p


@pytest.mark.parametrize("B,T", [(1, 64), (2, 68), (1, 65), (3, 32)])
def test_bf16_generator_matches_fp32_oracle(B, T):
    g, p = _gen(21)
    rs = np.random.RandomState(B * 1000 + T)
    x = torch.from_numpy(rs.randn(B, 80, T).astype(np.float32))
    m = torch.from_numpy(orc.fif_mask(rs, B, 80, T, min(25, T)))
    with torch.no_grad():
        ref = orc.generator_forward(p, x, m)
    got = g.infer(x.cuda(), m.cuda(), dtype="bf16")
    assert tuple(got.shape) == tuple(ref.shape)
    e = rel(got.cpu(), ref)
    print("bf16 generator (%d, %d): rel-L2 vs fp32 oracle %.3e" % (B, T, e))
    assert e < 2e-2, e
    # mask=None is the all-ones mask of test.py:92
    ones = g.infer(x.cuda(), None, dtype="bf16")
    ones2 = g.infer(x.cuda(), torch.ones_like(x).cuda(), dtype="bf16")
    assert torch.equal(ones, ones2)


def test_bf16_inference_config_bs16_512_frames():
    """BASELINE configs[4] at full size: bf16 vs the fp32 HIP forward (itself oracle-checked at this size by
    tests/test_hip_model.py) on all 16 samples, and vs the CPU oracle on sample 0; weights = seeded default init cast to bf16."""
    torch.manual_seed(0)
    g = Generator().cuda()
    gen = torch.Generator().manual_seed(1234)
    x = torch.randn(16, 80, 512, generator=gen).cuda()
    y32 = g.infer(x, None, dtype="f32")
    y16 = g.infer(x, None, dtype="bf16")
    e = rel(y16, y32)
    print("bf16 vs fp32 HIP at bs=16 x 512: rel-L2 %.3e" % e)
    assert e < 2e-2, e
    per_sample = [rel(y16[i], y32[i]) for i in range(16)]
    assert max(per_sample) < 3e-2, per_sample
    p = {k: v.detach().cpu() for k, v in g.state_dict().items()}
    with torch.no_grad():
        ref0 = orc.generator_forward(p, x[:1].cpu(), torch.ones(1, 80, 512))
    assert rel(y16[:1].cpu(), ref0) < 2e-2


def test_bf16_pack_follows_parameter_updates():
    g, p = _gen(23)
    x = torch.randn(1, 80, 64, device="cuda")
    y0 = g.infer(x, None, dtype="bf16").clone()
    with torch.no_grad():
        for q in g.parameters():
            q.mul_(1.01)                        # in-place update bumps the version counter -> re-pack
    y1 = g.infer(x, None, dtype="bf16")
    assert float((y1 - y0).abs().max()) > 1e-4
    g2 = Generator().cuda()
    g2.load_state_dict(g.state_dict())
    assert torch.equal(g2.infer(x, None, dtype="bf16"), y1)
