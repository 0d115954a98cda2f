"""GPU parity of the generator at the frame lengths inference, validation and training really use, against the oracle in float64.

The planner picks kernels by length (fused / persistent / staged-GEMM trunk, Winograd / implicit GEMM / fallback convolutions,
register / generic InstanceNorm, fused / unfused bf16 trunk), and ragged tiles go wrong at the edges of the time axis.  One
whole-tensor rel-L2 cannot see an error confined to a few frames (one frame 1e-2 off in 1004 is ~3e-4 overall), so every
comparison here also gates the worst (sample, frame) column of 80 mel values.

Gates are the project's bars, not measurements of one binary: fp32 <= 1e-3 whole and per frame; bf16 <= 2e-2 whole (as
test_hip_bf16.py) and <= 6e-2 per frame.

Below about 32 frames the network itself is ill-conditioned: InstanceNorm1d over W4 = T/4 <= 8 frames amplifies rounding, and at
W4 = 2 (T = 5..8) the reference's own fp32 arithmetic lands ~0.7 (rel-L2) away from the fp64 result.  No fp32 implementation can
meet 1e-3 there.  So for short inputs the test measures the reference's own spread at that input (the oracle in fp32, as the
reference runs; for bf16 the fp64 oracle on bf16-rounded weights and input) and applies the bar only where that spread is within
it; elsewhere the kernel must be no more than twice as far from fp64 as the reference is."""
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mcvc_oracle as orc  # noqa: E402  (checker only)
from mask_cyclegan_vc import _hip  # noqa: E402
from mask_cyclegan_vc.model import Generator  # noqa: E402

GATES = {"f32": (1e-3, 1e-3), "bf16": (2e-2, 6e-2)}        # (whole tensor, worst frame) rel-L2 vs the fp64 oracle
G_SEED = 11
MCVC_ERR_INVALID = 1001

LENGTHS = [
    5, 6, 7, 8,             # smallest valid lengths: T/4 (W4) = 2, the trunk's InstanceNorm1d over two frames
    12, 13,                 # W4 = 3 and 4: the lower edge (4 <= W4) of the persistent trunk backward
    31, 32, 33,             # the T >= 32 (and T % 4 == 0) edge of the Winograd-only weight pack
    63, 65, 66, 67,         # T = 3, 1, 2, 3 mod 4: Winograd / implicit GEMM need even or multiple-of-4 sizes, else the fallbacks
    100,                    # W4 = 25, odd; in the discriminator (W/2) & 3 != 0, so its implicit GEMM is skipped
    128, 129, 132,          # fused fp32 trunk at W4 = 32 (B*W4 <= 64, W4 <= 32), then past it: the staged-GEMM trunk at bs 1
    320,                    # validation default (--num_frames_validation)
    511, 512, 513, 516,     # bf16 kTrunkMaxW = 128: fused bf16 trunk / conv2dto1d+norm up to W4 = 128, unfused above
    1001, 1601,             # long utterances: InstanceNorm over P > 5120 points on the generic kernels, unfused bf16 trunk
]
BATCH_LENGTHS = [65, 132, 513]   # bs 3 vs each sample's own bs-1 result: ragged / fused / unfused bf16 trunk


def frame_errors(got, ref):
    """Per (sample, frame) column of 80 mel values: ||got - ref|| / max(||ref||, floor) -> [B, T'].  The floor (a tenth of the
    sample's RMS frame norm) only guards near-silent frames; the generator's output frames sit far above it."""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    num = (got - ref).norm(dim=1)
    den = ref.norm(dim=1)
    floor = 0.1 * den.pow(2).mean(dim=1, keepdim=True).sqrt()
    return num / torch.maximum(den, floor)


def whole_error(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float((got - ref).norm() / max(float(ref.norm()), 1e-30))


def check(tag, dtype, got, ref, spread=None):
    """Assert both gates of ``dtype``; print the measured values (and where the worst frame is).  ``spread``: (whole, worst frame)
    error of the reference's own arithmetic at this input (``reference_spread``); where it exceeds the bar the gate is twice it."""
    assert tuple(got.shape) == tuple(ref.shape), (tag, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(torch.as_tensor(got)).all(), tag
    whole_gate, frame_gate = GATES[dtype]
    note = ""
    if spread is not None and (spread[0] > whole_gate or spread[1] > frame_gate):
        whole_gate, frame_gate = max(whole_gate, 2 * spread[0]), max(frame_gate, 2 * spread[1])
        note = "  [ill-conditioned: reference's own %s error %.3e / %.3e]" % (dtype, spread[0], spread[1])
    fe = frame_errors(got, ref)
    whole, worst = whole_error(got, ref), float(fe.max())
    b, t = divmod(int(fe.argmax()), fe.shape[1])
    print("%-26s %-4s whole %.3e  worst frame %.3e (sample %d, frame %d of %d)%s" % (tag, dtype, whole, worst, b, t, fe.shape[1], note))
    assert whole <= whole_gate, (tag, dtype, "whole", whole, whole_gate)
    assert worst <= frame_gate, (tag, dtype, "frame", worst, frame_gate, b, t)


def reference_spread(x, ref, T):
    """{dtype: (whole, worst frame)} error vs the fp64 oracle of the reference's own arithmetic on input ``x``: the oracle in fp32
    (what the reference computes) and, as the bf16 counterpart, the fp64 oracle on bf16-rounded weights and input.  None from 33
    frames up, where both are far inside the bars (measured at T = 64: 1.3e-6 and 8.5e-3 whole)."""
    if T > 33:
        return {"f32": None, "bf16": None}
    out = {}
    with torch.no_grad():
        gp32 = orc.filler_params("G", G_SEED)
        out["f32"] = orc.generator_forward(gp32, x, torch.ones_like(x))
        gpbf = {k: v.to(torch.bfloat16).double() for k, v in gp32.items()}
        xb = x.to(torch.bfloat16).double()
        out["bf16"] = orc.generator_forward(gpbf, xb, torch.ones_like(xb))
    return {k: (whole_error(v, ref), float(frame_errors(v, ref).max())) for k, v in out.items()}


def inputs(B, T, seed):
    return torch.from_numpy(np.random.RandomState(seed).randn(B, 80, T).astype(np.float32))


def oracle(gp64, x):
    with torch.no_grad():
        x = x.double()
        return orc.generator_forward(gp64, x, torch.ones_like(x))


@pytest.fixture(scope="module")
def gp64():
    return orc.filler_params("G", G_SEED, dtype=torch.float64)      # cast from the fp32 draw: both sides see identical values


@pytest.fixture(scope="module")
def gen():
    g = Generator()
    g.load_state_dict(orc.filler_params("G", G_SEED), strict=True)
    return g.cuda()


def forwards(g, x):
    """infer f32, the autograd forward (all-ones mask, parameters requiring grad) and infer bf16 of one input, on the GPU."""
    xc = x.cuda()
    with torch.no_grad():
        f32 = g.infer(xc, None, "f32").cpu()
        bf16 = g.infer(xc, None, "bf16").cpu()
    fwd = g(xc, torch.ones_like(xc))
    assert fwd.requires_grad
    return f32, fwd.detach().cpu(), bf16


@pytest.mark.parametrize("T", LENGTHS)
def test_generator_forward_at_length(T, gen, gp64):
    """bs 1: infer f32, the autograd forward and infer bf16 vs the fp64 oracle; output length = the oracle's; infer f32 == forward
    bit for bit (Generator.infer's promise)."""
    x = inputs(1, T, 1000 + T)
    ref = oracle(gp64, x)
    assert ref.shape[2] == _hip.lib().mcvc_gen_out_frames(T)
    spread = reference_spread(x, ref, T)
    f32, fwd, bf16 = forwards(gen, x)
    assert torch.equal(f32, fwd), ("infer f32 != forward", T, float((f32 - fwd).abs().max()))
    check("T=%d infer" % T, "f32", f32, ref, spread["f32"])
    check("T=%d forward" % T, "f32", fwd, ref, spread["f32"])
    check("T=%d infer" % T, "bf16", bf16, ref, spread["bf16"])


@pytest.mark.parametrize("T", BATCH_LENGTHS)
def test_generator_batch_of_three_at_length(T, gen, gp64):
    """bs 3 (three different utterances of one length, as the inference driver batches them): every sample vs the fp64 oracle and
    vs its own bs-1 result, under the same gates."""
    x = inputs(3, T, 2000 + T)
    ref = oracle(gp64, x)
    batched = forwards(gen, x)
    single = [forwards(gen, x[i:i + 1]) for i in range(3)]
    for name, dtype, k in (("infer", "f32", 0), ("forward", "f32", 1), ("infer", "bf16", 2)):
        check("T=%d bs3 %s" % (T, name), dtype, batched[k], ref)
        for i in range(3):
            check("T=%d bs3 %s [%d] vs bs1" % (T, name, i), dtype, batched[k][i:i + 1], single[i][k])


@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_tiny_inputs_are_refused_like_the_reference(T, gen, gp64):
    """T <= 4 leaves one frame after the two stride-2 convolutions: the reference's InstanceNorm1d raises there.  Every generator
    entry point refuses too (MCVC_ERR_INVALID) instead of returning numbers -- forward, both inference dtypes and the backward."""
    x = inputs(1, T, 3000 + T)
    with pytest.raises(ValueError, match="more than 1 spatial element"):
        oracle(gp64, x)
    xc = x.cuda()
    with pytest.raises(RuntimeError, match="mcvc_gen_forward failed with code %d" % MCVC_ERR_INVALID):
        gen(xc, torch.ones_like(xc))
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="mcvc_gen_forward failed with code %d" % MCVC_ERR_INVALID):
            gen.infer(xc, None, "f32")
        with pytest.raises(RuntimeError, match="mcvc_gen_infer_bf16 failed with code %d" % MCVC_ERR_INVALID):
            gen.infer(xc, None, "bf16")
    # the backward entries, on buffers sized for this (B, T): refused before anything is read
    L = _hip.lib()
    ps = gen._plist()
    packed = gen.packed_weights(ps)
    stash = torch.zeros(L.mcvc_gen_stash_floats(1, T), device="cuda")
    scratch = torch.zeros(L.mcvc_gen_scratch_floats(1, T), device="cuda")
    dout = torch.ones(1, 80, L.mcvc_gen_out_frames(T), device="cuda")
    dx = torch.zeros_like(xc)
    grads = [torch.zeros_like(p) for p in ps]
    ones = torch.ones_like(xc)
    P, G = _hip.ptr_table(ps), _hip.ptr_table(grads)
    args = (_hip.ptr(ones), _hip.ptr(dout), _hip.ptr(dx), 0, _hip.ptr(stash))
    tail = (_hip.ptr(scratch), scratch.numel(), 1, T, _hip.stream())
    assert L.mcvc_gen_backward(P, _hip.ptr(packed), G, *args, *tail, None) == MCVC_ERR_INVALID
    assert L.mcvc_gen_backward_flags(P, _hip.ptr(packed), G, *args, *tail, None, None, 0) == MCVC_ERR_INVALID
    assert L.mcvc_gen_backward_window(P, _hip.ptr(packed), G, *args, 1, 0, *tail, None, None, 0) == MCVC_ERR_INVALID
    torch.cuda.synchronize()
    assert float(dx.abs().sum()) == 0.0 and all(float(g.abs().sum()) == 0.0 for g in grads)


CLI_LENGTHS = [5, 13, 63, 65, 65, 65, 66, 67, 130, 320, 513, 513, 1001]


def test_inference_cli_at_utterance_lengths(tmp_path, gp64):
    """python -m mask_cyclegan_vc.test with --max_batch 2 over one speaker's utterances of ragged lengths: the 65-frame bucket of
    three runs as batches of 2 + 1, and the ten (B, T) shapes on two streams make the per-stream workspace cache (at most four)
    evict while both streams have work in flight.  Every written mel, normalised back, vs the fp64 oracle's conversion."""
    from mask_cyclegan_vc import test as test_cli
    data = str(tmp_path / "data")
    rs = np.random.RandomState(4)
    mels = {"SPKA": [rs.randn(80, T).astype(np.float32) for T in CLI_LENGTHS], "SPKB": [rs.randn(80, 64).astype(np.float32)]}
    stat = {}
    for spk, ms in mels.items():
        os.makedirs(os.path.join(data, spk))
        with open(os.path.join(data, spk, "%s_normalized.pickle" % spk), "wb") as fh:
            pickle.dump(ms, fh)
        stat[spk] = dict(mean=rs.randn(80, 1).astype(np.float32), std=(1 + rs.rand(80, 1)).astype(np.float32))
        np.savez(os.path.join(data, spk, "%s_norm_stat.npz" % spk), **stat[spk])
    ck = tmp_path / "ckpts"
    ck.mkdir()
    torch.save({"ckpt_info": {"epoch": 1}, "model_class": "Generator", "model_state": orc.filler_params("G", G_SEED), "optimizer": None,
                "lr_scheduler": None}, str(ck / "00001_generator_A2B.pth.tar"))
    refs, spreads = [], []
    for m in mels["SPKA"]:
        x = torch.from_numpy(m)[None]
        refs.append(oracle(gp64, x)[0])
        spreads.append(reference_spread(x, refs[-1][None], x.shape[2]))
    mean, std = stat["SPKB"]["mean"].astype(np.float64), stat["SPKB"]["std"].astype(np.float64)     # de-normalised with the TARGET's
    for dtype in ("f32", "bf16"):
        test_cli.main(["--name", "len_" + dtype, "--save_dir", str(tmp_path / "res"), "--preprocessed_data_dir", data, "--speaker_A_id", "SPKA",
                       "--speaker_B_id", "SPKB", "--ckpt_dir", str(ck), "--load_epoch", "1", "--model_name", "generator_A2B", "--dtype", dtype,
                       "--max_batch", "2"])
        out = str(tmp_path / "res" / ("len_" + dtype) / "converted_mel")
        assert len(os.listdir(out)) == len(CLI_LENGTHS)
        for i, (T, ref, spread) in enumerate(zip(CLI_LENGTHS, refs, spreads)):
            got = (np.load(os.path.join(out, "%d-converted_SPKA_to_SPKB.npy" % i)).astype(np.float64) - mean) / std
            check("CLI utterance %d T=%d" % (i, T), dtype, got[None], ref[None], spread[dtype])


def _wino_gemm_launches(fn):
    from test_hip_model import _launches
    return _launches("wino_gemm", fn)


def test_generator_batch_of_five_long_utterances_runs_chunked_winograd_passes(gen, gp64):
    """bs 5 at T = 660 (T/4 = 165, odd): upSample2 and downSample1 have 20 x 165 = 3300 2x2 tiles per sample and no 4x4 form (330 columns), so
    their Winograd passes hold 16384 / 3300 = 4 samples at most and run as chunks of 3 + 2 samples -- forward, data gradient and weight
    gradient.  Every sample of infer f32 and of the autograd forward vs its own bs-1 result; samples 0 and 4 (one of each chunk) vs the fp64
    oracle; with a seeded dout the batch's parameter gradients and dx vs the sum, respectively the stack, of the five bs-1 backward passes
    (1e-4 of each tensor's norm, the gate of test_backward_over_a_window_of_the_forward_samples; the conv biases in front of an InstanceNorm,
    whose gradient is rounding noise below 1e-4, are skipped).  The launch trace proves the regime: the batch's forward makes more Winograd
    GEMM launches (6: two layers in two chunks) than a bs-1 forward of the same length (4)."""
    B, T = 5, 660
    x = inputs(B, T, 4000 + T)
    xc = x.cuda()
    params = gen._plist()

    def run(xs, dout):
        """infer f32, the autograd forward, and its backward's dx; the parameter gradients accumulate in .grad"""
        with torch.no_grad():
            f32 = gen.infer(xs, None, "f32").cpu()
        xg = xs.clone().requires_grad_(True)
        fwd = gen(xg, torch.ones_like(xs))
        fwd.backward(dout)
        return f32, fwd.detach().cpu(), xg.grad.cpu()

    dout = torch.randn(B, 80, _hip.lib().mcvc_gen_out_frames(T), generator=torch.Generator().manual_seed(4001)).cuda()
    try:
        for p in params:
            p.grad = None
        b_f32, b_fwd, b_dx = run(xc, dout)
        b_grads = [p.grad.detach().cpu().double() for p in params]
        for p in params:
            p.grad = None
        single = [run(xc[i:i + 1], dout[i:i + 1]) for i in range(B)]
        s_grads = [p.grad.detach().cpu().double() for p in params]
    finally:
        for p in params:
            p.grad = None

    assert torch.equal(b_f32, b_fwd), ("infer f32 != forward", float((b_f32 - b_fwd).abs().max()))
    for name, got, k in (("infer", b_f32, 0), ("forward", b_fwd, 1)):
        for i in range(B):
            check("T=%d bs5 %s [%d] vs bs1" % (T, name, i), "f32", got[i:i + 1], single[i][k])
    for i in (0, B - 1):                                   # one sample of each chunk
        ref = oracle(gp64, x[i:i + 1])
        check("T=%d bs5 infer [%d] vs fp64" % (T, i), "f32", b_f32[i:i + 1], ref)
        check("T=%d bs5 forward [%d] vs fp64" % (T, i), "f32", b_fwd[i:i + 1], ref)

    s_dx = torch.cat([s[2] for s in single], 0).double()
    e_dx = float((b_dx.double() - s_dx).norm() / s_dx.norm())
    print("T=%d bs5 backward: dx vs the stacked bs-1 passes %.3e" % (T, e_dx))
    assert e_dx <= 1e-4, e_dx
    worst, compared = 0.0, 0
    names = [n for n, _ in gen.named_parameters()]
    for i, (a_, b_) in enumerate(zip(b_grads, s_grads)):
        nb_ = float(b_.norm())
        if nb_ < 1e-4:                                     # conv biases in front of an InstanceNorm: mathematically zero
            continue
        e = float((a_ - b_).norm()) / nb_
        worst, compared = max(worst, e), compared + 1
        assert e <= 1e-4, (names[i], e)
    print("T=%d bs5 backward: %d parameter gradients vs the sum of the bs-1 passes, worst %.3e" % (T, compared, worst))
    assert compared > 40

    with torch.no_grad():
        n_batch = _wino_gemm_launches(lambda: gen.infer(xc, None, "f32"))
        n_single = _wino_gemm_launches(lambda: gen.infer(xc[:1], None, "f32"))
    print("T=%d Winograd GEMM launches per forward: bs5 %d, bs1 %d" % (T, n_batch, n_single))
    assert n_batch > n_single > 0, (n_batch, n_single)
