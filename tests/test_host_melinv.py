"""CPU-only checks of the mel inversion's host side (mask_cyclegan_vc/melinv.py, the mcvc_melinv_* C ABI): symbols, the tables
against restatements, the refusals of a basis without the sparse structure, the command-line rules, and the float64 checker
(melinv_checker.py) against the figures the method was chosen on.  No kernel is launched here."""
import os
import re

import numpy as np
import pytest

import griffinlim_checker as glck
import melinv_checker as ck
from args.cycleGAN_test_arg_parser import CycleGANTestArgParser
from data_preprocessing.audio2mel import mel_filterbank, read_wav
from mask_cyclegan_vc import _hip, melinv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCVC_ERR_INVALID = 1001
NBIN, NMEL, LD = 513, 80, 516
OFF_STEP = NBIN * NMEL
OFF_BETA = OFF_STEP + 4
OFF_CST = OFF_BETA + 512
C_W0, C_W1, C_FILT, C_FW = LD, 2 * LD, 3 * LD, 3 * LD + 4 * NMEL
SYMBOLS = ("mcvc_melinv_max_iter", "mcvc_melinv_tables_floats", "mcvc_melinv_tables_init", "mcvc_melinv_solve")


@pytest.fixture(scope="module")
def tables():
    return melinv.host_tables()


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "mcvc.h")).read()
    declared = set(re.findall(r"\b(mcvc_[a-z0-9_]+)\s*\(", header))
    L = _hip.lib()
    for name in SYMBOLS:
        assert name in declared and name in _hip.EXPORTED_SYMBOLS and getattr(L, name).argtypes is not None, name
    assert L.mcvc_version() == 3
    assert L.mcvc_melinv_max_iter() == 512 == melinv.MAX_ITER == ck.MAX_ITER
    assert L.mcvc_melinv_tables_floats() == OFF_CST + C_FW + 1028


def test_tables_against_the_checker(tables):
    B32 = mel_filterbank(np.float64).astype(np.float32)
    same = int((B32 == ck.basis().astype(np.float32)).sum())
    print("basis: %d of %d float32 entries equal the checker's scalar-loop basis" % (same, B32.size))
    assert np.abs(mel_filterbank(np.float64) - ck.basis()).max() <= 1e-12 * np.abs(ck.basis()).max()
    from mask_cyclegan_vc.griffinlim import pinv_mel_basis
    assert np.array_equal(tables[:OFF_STEP].reshape(NBIN, NMEL), pinv_mel_basis().astype(np.float32))      # the decoder's table
    assert np.abs(pinv_mel_basis() - ck.pinv_basis()).max() <= 1e-10
    lam = melinv.lipschitz()
    print("lambda = %.6e (checker %.6e)" % (lam, ck.lipschitz()))
    assert abs(lam - ck.lipschitz()) <= 1e-12 * lam and abs(lam - 1.128e-3) < 1e-6
    assert tables[OFF_STEP] == np.float32(1.0 / lam)
    assert np.array_equal(tables[OFF_BETA:OFF_CST], ck.betas(512).astype(np.float32))
    assert tables[OFF_BETA] == 0.0 and 0.0 < tables[OFF_BETA + 1] < tables[OFF_BETA + 511] < 1.0
    # the sparse tables, put back together, are the basis: once from the bins' side, once from the filters' side
    cst = tables[OFF_CST:]
    first, w0, w1 = cst[:LD].view(np.int32), cst[C_W0:C_W0 + LD], cst[C_W1:C_W1 + LD]
    filt = cst[C_FILT:C_FILT + 4 * NMEL].view(np.int32).reshape(NMEL, 4)
    by_bin, by_filter = np.zeros((NMEL, NBIN), np.float32), np.zeros((NMEL, NBIN), np.float32)
    for b in range(NBIN):
        if first[b] >= 0:
            assert first[b] + 1 < NMEL
            by_bin[first[b], b], by_bin[first[b] + 1, b] = w0[b], w1[b]
    assert first[0] == -1 and first[512] == -1 and (first[1:512] >= 0).all() and (first[NBIN:] == -1).all()
    off = 0
    for j in range(NMEL):
        fb, cnt, o = filt[j, :3]
        assert o == off and 1 <= cnt <= 41 and fb + cnt <= NBIN
        by_filter[j, fb:fb + cnt] = cst[C_FW + o:C_FW + o + cnt]
        off += cnt
    assert off <= 2 * NBIN
    assert np.array_equal(by_bin, B32) and np.array_equal(by_filter, B32)


def test_tables_init_refuses_a_basis_without_the_structure(tables):
    L = _hip.lib()
    B = mel_filterbank(np.float64).astype(np.float32)
    from mask_cyclegan_vc.griffinlim import pinv_mel_basis
    P = np.ascontiguousarray(pinv_mel_basis(), dtype=np.float32)
    lam = melinv.lipschitz()
    out = np.full(L.mcvc_melinv_tables_floats(), 7.0, dtype=np.float32)
    call = lambda basis, p=P, l=lam, o=out: L.mcvc_melinv_tables_init(None if basis is None else basis.ctypes.data, None if p is None else p.ctypes.data,
                                                                        l, None if o is None else o.ctypes.data)
    three = B.copy()
    b = 300
    j = int(np.nonzero(B[:, b])[0][0])
    assert np.count_nonzero(B[:, b]) == 2
    three[j + 2, b] = 1e-3                                   # a third non-zero next to the pair
    apart = B.copy()
    apart[j + 1, b] = 0.0
    apart[j + 2, b] = 1e-3                                   # a pair with a filter between
    hole = B.copy()
    fb = np.nonzero(B[79])[0]
    hole[79, fb[len(fb) // 2]] = 0.0                         # a filter whose non-zeros are not contiguous
    nan = B.copy()
    nan[3, 7] = np.nan
    for name, bad in (("three non-zeros", three), ("non-adjacent pair", apart), ("filter with a hole", hole), ("nan", nan)):
        assert call(bad) == MCVC_ERR_INVALID, name
    for lam_bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(B, l=lam_bad) == MCVC_ERR_INVALID, lam_bad
    assert call(None) == MCVC_ERR_INVALID and call(B, p=None) == MCVC_ERR_INVALID and call(B, o=None) == MCVC_ERR_INVALID
    assert (out == 7.0).all()                                # a refused call writes nothing
    assert call(B) == 0 and np.array_equal(out.view(np.int32), tables.view(np.int32))
    single = B.copy()                                        # allowed: a column with one non-zero, in the first or the last filter
    single[:, 1] = 0.0
    single[0, 1] = B[0, 1]
    single[:, 511] = 0.0
    single[79, 511] = B[79, 511]
    assert call(single) == 0
    with pytest.raises(RuntimeError, match="mcvc_melinv_tables_init"):
        melinv.host_tables(basis=three)


def test_solve_refuses_before_it_touches_a_device():
    L = _hip.lib()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    assert L.mcvc_melinv_solve(p, p, p, 1, 0, 8, None) == MCVC_ERR_INVALID            # T = 0
    assert L.mcvc_melinv_solve(p, p, p, 0, 4, 8, None) == MCVC_ERR_INVALID            # B = 0
    assert L.mcvc_melinv_solve(p, p, p, 1, 4, -1, None) == MCVC_ERR_INVALID           # n_iter < 0
    assert L.mcvc_melinv_solve(p, p, p, 1, 4, 513, None) == MCVC_ERR_INVALID          # n_iter beyond the maximum
    assert L.mcvc_melinv_solve(None, p, p, 1, 4, 8, None) == MCVC_ERR_INVALID
    assert L.mcvc_melinv_solve(p, None, p, 1, 4, 8, None) == MCVC_ERR_INVALID
    assert L.mcvc_melinv_solve(p, p, None, 1, 4, 8, None) == MCVC_ERR_INVALID
    assert L.mcvc_melinv_solve(p + 2, p, p, 1, 4, 8, None) == MCVC_ERR_INVALID        # misaligned
    assert L.mcvc_melinv_solve(p, p + 4, p, 1, 4, 8, None) == MCVC_ERR_INVALID        # tables off the 16-byte boundary
    assert L.mcvc_melinv_solve(p, p, p + 1, 1, 4, 8, None) == MCVC_ERR_INVALID
    assert L.mcvc_melinv_solve(p, p, p, 65536, 1, 8, None) == MCVC_ERR_INVALID        # the decoder's limits
    assert L.mcvc_melinv_solve(p, p, p, 1, (1 << 20) + 1, 8, None) == MCVC_ERR_INVALID
    assert L.mcvc_melinv_solve(p, p, p, 8, 1 << 20, 8, None) == MCVC_ERR_INVALID      # B T > 2^22
    assert (buf == 0).all()


def test_flags(tmp_path):
    base = ["--save_dir", str(tmp_path), "--name", "r", "--ckpt_dir", str(tmp_path), "--load_epoch", "1"]
    for bad in (["--gl_mel_inverse", "nnls"], ["--gl_mel_inverse", "pinv"], ["--gl_mel_iter", "8"],
                ["--griffin_lim", "0", "--gl_mel_inverse", "nnls"], ["--vocoder_ckpt", "melgan.pt", "--gl_mel_iter", "8"],
                ["--griffin_lim", "4", "--gl_mel_iter", "-1"], ["--griffin_lim", "4", "--gl_mel_iter", "513"],
                ["--griffin_lim", "4", "--gl_mel_inverse", "lbfgs"], ["--griffin_lim", "4", "--gl_mel_iter", "many"]):
        with pytest.raises(SystemExit):
            CycleGANTestArgParser().parse_args(base + bad)
    assert not (tmp_path / "r").exists()                     # refused before the run directory is made
    a = CycleGANTestArgParser().parse_args(base)
    assert a.griffin_lim == 0 and a.gl_mel_inverse == "pinv" and a.gl_mel_iter == 64
    a = CycleGANTestArgParser().parse_args(base + ["--griffin_lim", "4"])
    assert a.griffin_lim == 4 and a.gl_mel_inverse == "pinv" and a.gl_mel_iter == 64
    a = CycleGANTestArgParser().parse_args(base + ["--griffin_lim", "4", "--gl_mel_inverse", "nnls"])
    assert a.gl_mel_inverse == "nnls" and a.gl_mel_iter == 64
    for n in (0, 8, 512):
        a = CycleGANTestArgParser().parse_args(base + ["--griffin_lim", "4", "--gl_mel_inverse", "nnls", "--gl_mel_iter", str(n)])
        assert a.gl_mel_inverse == "nnls" and a.gl_mel_iter == n
    p = CycleGANTestArgParser()                              # one parser, two command lines: the second does not inherit the first's flags
    p.parse_args(base + ["--griffin_lim", "4", "--gl_mel_iter", "8"])
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--gl_mel_iter", "8"])


def test_module_refuses_bad_settings_and_has_no_cpu_path():
    import torch
    from mask_cyclegan_vc import griffinlim
    for bad in (-1, 513):
        with pytest.raises(ValueError):
            melinv.check_n_iter(bad)
    assert melinv.check_n_iter(0) == 0 and melinv.check_n_iter(512) == 512
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            melinv.MelInverter()
        with pytest.raises(RuntimeError, match="no CPU path"):
            griffinlim.GriffinLimVocoder(mel_inverse="nnls")


@pytest.mark.parametrize("clip", ["real_VCC2SF3.wav", "real_VCC2TF1.wav"])
def test_checker_against_the_cpu_measurements(golden_dir, clip):
    """The float64 checker on a committed recording, from the log-mel of the front-end's own STFT magnitude S, at 32 iterations:
    mel residual <= 1 / 10 of the clamp's (measured: 1 / 800 and 1 / 250) and || M - S || / || S || <= 0.9 x the clamp's (measured:
    0.74 and 0.78).  Conditions on the method, with wide margin; the start value is the decoder checker's magnitude."""
    x = read_wav(os.path.join(golden_dir, "audio", clip)).astype(np.float64)
    S = glck.stft(x[None]).abs().numpy()                     # [1, 513, T]
    logmel = np.log10(np.maximum(np.einsum("jb,nbt->njt", ck.basis(), S), 1e-5))
    M0, M32 = ck.solve(logmel, 0), ck.solve(logmel, 32)
    assert np.array_equal(M0, ck.start(logmel)) and (M32 >= 0).all()
    ref = glck.magnitude_from_mel(logmel).numpy()            # the unrounded pinv: the two start values differ by the table's rounding
    assert np.abs(M0 - ref).max() <= 1e-5 * np.abs(ref).max()
    res0, res32 = ck.mel_residual(M0, logmel), ck.mel_residual(M32, logmel)
    d0, d32 = ck.relative_distance(M0, S), ck.relative_distance(M32, S)
    print("%s T=%d: mel residual clamp %.3e, 32 iterations %.3e (ratio 1 / %.0f);  ||M - S|| / ||S|| clamp %.4f, 32 iterations %.4f (ratio %.3f)"
          % (clip, S.shape[2], res0, res32, res0 / res32, d0, d32, d32 / d0))
    assert res32 <= res0 / 10.0
    assert d32 <= 0.9 * d0
