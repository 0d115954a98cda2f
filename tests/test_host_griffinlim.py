"""CPU-only checks of the Griffin-Lim decoder's host side (mask_cyclegan_vc/griffinlim.py, the mcvc_gl_* C ABI): the pseudo-inverse of
the mel basis and the inverse DFT basis against restatements, the size laws, the command-line flag, and the checker's own round trip.
No kernel is launched here."""
import numpy as np
import pytest
import torch

import griffinlim_checker as ck
from args.cycleGAN_test_arg_parser import CycleGANTestArgParser
from mask_cyclegan_vc import _hip, griffinlim

MCVC_ERR_INVALID, MCVC_ERR_WORKSPACE = 1001, 1002
N, NBIN, NMEL = 1024, 513, 80
OFF_PINV, OFF_W2, OFF_FWD = N * N, N * N + NBIN * NMEL, N * N + NBIN * NMEL + N
GL_SYMBOLS = ("mcvc_gl_out_samples", "mcvc_gl_launches", "mcvc_gl_tables_floats", "mcvc_gl_tables_init", "mcvc_gl_workspace_floats", "mcvc_gl_decode")


@pytest.fixture(scope="module")
def tables():
    return griffinlim.host_tables()


def undo_lane_order(a):
    """float index ((mt * 128 + kg) * 64 + lane) * 4 + j  ->  X[row 32 mt + (lane & 31)][k = 8 kg + 2 j + (lane >> 5)]."""
    a = np.asarray(a).reshape(32, 128, 64, 4)
    X = np.full((N, N), np.nan, dtype=a.dtype)
    mt, kg = np.arange(32)[:, None], np.arange(128)[None, :]
    for lane in range(64):
        for j in range(4):
            X[32 * mt + (lane & 31), 8 * kg + 2 * j + (lane >> 5)] = a[:, :, lane, j]
    return X


def test_pinv_table_against_the_checker(tables):
    P, want = griffinlim.pinv_mel_basis(), ck.pinv_basis()
    assert P.shape == (NBIN, NMEL) and P.dtype == np.float64
    err = float(np.abs(P - want).max())
    print("pinv: max abs difference %.3e (largest entry %.3e)" % (err, float(np.abs(want).max())))
    assert err <= 1e-10
    assert np.array_equal(tables[OFF_PINV:OFF_W2].reshape(NBIN, NMEL), P.astype(np.float32))      # the caller's table, taken as it is


def test_inverse_basis_fill_against_numpy(tables):
    """IB[n][slot]: frame[n] = sum over the packed spectrum slots; slot 2b / 2b + 1 = Re / Im of bin b, slot 1 = Re of bin 512."""
    L = _hip.lib()
    assert L.mcvc_gl_tables_floats() == OFF_FWD + L.mcvc_audio_basis_floats() and tables.size == L.mcvc_gl_tables_floats()
    IB = undo_lane_order(tables[:N * N])
    assert np.isfinite(IB).all()
    n = np.arange(N)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / N)
    want = np.zeros((N, N))
    want[:, 0] = w / N
    want[:, 1] = w * np.where(n % 2 == 0, 1.0, -1.0) / N
    for b in range(1, 512):
        ph = 2.0 * np.pi * ((n * b) % N) / N                   # exact argument reduction
        want[:, 2 * b] = 2.0 * w * np.cos(ph) / N
        want[:, 2 * b + 1] = -2.0 * w * np.sin(ph) / N
    err = float(np.abs(IB.astype(np.float64) - want).max())
    print("inverse basis: max abs difference %.3e (one float32 ulp of the largest entry: %.3e)" % (err, 2.0 ** -23 * 2.0 / N))
    assert err <= 2.0 ** -23 * 2.0 / N                          # float32 rounding of values up to 2 / 1024, cos / sin of two libraries
    # as an operator: the basis applied to the packed rfft of a windowed frame gives w * irfft, i.e. w^2 * frame
    x = np.random.RandomState(0).randn(N)
    S = np.fft.rfft(w * x)
    packed = np.zeros(N)
    packed[0], packed[1], packed[2::2], packed[3::2] = S[0].real, S[512].real, S[1:512].real, S[1:512].imag
    assert np.abs(IB.astype(np.float64) @ packed - w * w * x).max() <= 1e-5
    # the squared window and the front-end's operand
    assert np.abs(tables[OFF_W2:OFF_FWD] - w * w).max() <= 2.0 ** -24              # float32 rounding of values up to 1
    fwd = np.empty(L.mcvc_audio_basis_floats(), dtype=np.float32)
    assert L.mcvc_audio_basis_init(fwd.ctypes.data) == 0
    assert np.array_equal(tables[OFF_FWD:].view(np.int32), fwd.view(np.int32))
    assert L.mcvc_gl_tables_init(None, tables.ctypes.data) == MCVC_ERR_INVALID
    assert L.mcvc_gl_tables_init(tables.ctypes.data, None) == MCVC_ERR_INVALID


def test_size_laws():
    L = _hip.lib()
    for T in (-1, 0, 1):
        assert L.mcvc_gl_out_samples(T) == 0 and L.mcvc_gl_workspace_floats(1, T) == 0
    assert L.mcvc_gl_workspace_floats(0, 8) == 0
    assert L.mcvc_gl_out_samples(2) == 512 and L.mcvc_gl_out_samples(512) == 131072
    assert L.mcvc_gl_launches(-1) == 0 and L.mcvc_gl_launches(0) == 3 and L.mcvc_gl_launches(32) == 67
    prev_s = prev_l = 0
    for T in (2, 3, 4, 7, 64, 65, 129, 512):
        assert L.mcvc_gl_out_samples(T) == 256 * T > prev_s
        prev_s = L.mcvc_gl_out_samples(T)
        prev_b = 0
        for B in (1, 2, 3, 16):
            cur = L.mcvc_gl_workspace_floats(B, T)
            assert cur > prev_b and cur >= B * T * (2 * N + N + NBIN) and cur % 2 == 0
            prev_b = cur
        assert L.mcvc_gl_workspace_floats(1, T) > prev_l
        prev_l = L.mcvc_gl_workspace_floats(1, T)
    for n in range(0, 40):
        assert L.mcvc_gl_launches(n + 1) > L.mcvc_gl_launches(n)


def test_decode_refuses_before_it_touches_a_device():
    """Every refusal comes from the argument check: no device is needed to see it (the pointers are never followed)."""
    L = _hip.lib()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    n = L.mcvc_gl_workspace_floats(1, 2)
    assert L.mcvc_gl_decode(p, 0, None, p, p, p, n, 1, 1, 0, 0.99, None) == MCVC_ERR_INVALID          # T = 1
    assert L.mcvc_gl_decode(p, 0, None, p, p, p, n, 0, 2, 0, 0.99, None) == MCVC_ERR_INVALID          # B = 0
    assert L.mcvc_gl_decode(p, 0, None, p, p, p, n, 1, 2, -1, 0.99, None) == MCVC_ERR_INVALID         # n_iter < 0
    assert L.mcvc_gl_decode(p, 0, None, p, p, p, n, 1, 2, 0, 1.0, None) == MCVC_ERR_INVALID           # momentum 1
    assert L.mcvc_gl_decode(p, 0, None, p, p, p, n, 1, 2, 0, -0.1, None) == MCVC_ERR_INVALID
    assert L.mcvc_gl_decode(p, 2, None, p, p, p, n, 1, 2, 0, 0.5, None) == MCVC_ERR_INVALID           # unknown input kind
    assert L.mcvc_gl_decode(None, 0, None, p, p, p, n, 1, 2, 0, 0.5, None) == MCVC_ERR_INVALID
    assert L.mcvc_gl_decode(p, 0, None, p + 4, p, p, n, 1, 2, 0, 0.5, None) == MCVC_ERR_INVALID       # tables off the 16-byte boundary
    assert L.mcvc_gl_decode(p, 0, None, p, p, p, n - 1, 1, 2, 0, 0.5, None) == MCVC_ERR_WORKSPACE
    assert L.mcvc_gl_decode(p, 0, None, p, p, None, n, 1, 2, 0, 0.5, None) == MCVC_ERR_WORKSPACE


def test_griffin_lim_flag(tmp_path):
    p = CycleGANTestArgParser().parser                       # (the bare parser: parse_args of the wrapper creates run directories)
    assert p.parse_args([]).griffin_lim == 0
    assert p.parse_args(["--griffin_lim", "8"]).griffin_lim == 8
    with pytest.raises(SystemExit):
        p.parse_args(["--griffin_lim", "many"])
    base = ["--save_dir", str(tmp_path), "--name", "r", "--ckpt_dir", str(tmp_path), "--load_epoch", "1"]
    for bad in (["--griffin_lim", "8", "--vocoder_ckpt", "melgan.pt"], ["--griffin_lim", "-1"]):
        with pytest.raises(SystemExit):
            CycleGANTestArgParser().parse_args(base + bad)
    assert not (tmp_path / "r").exists()                     # refused before the run directory is made
    a = CycleGANTestArgParser().parse_args(base + ["--griffin_lim", "8"])
    assert a.griffin_lim == 8 and a.vocoder_ckpt is None
    assert CycleGANTestArgParser().parse_args(base + ["--vocoder_ckpt", "melgan.pt"]).griffin_lim == 0


def test_symbols_are_bound():
    L = _hip.lib()
    for name in GL_SYMBOLS:
        assert name in _hip.EXPORTED_SYMBOLS and getattr(L, name).argtypes is not None
    assert L.mcvc_version() == 3


def test_module_refuses_bad_settings_and_has_no_cpu_path():
    if torch.cuda.is_available():
        with pytest.raises(ValueError):
            griffinlim.GriffinLimVocoder(momentum=1.0)
        with pytest.raises(ValueError):
            griffinlim.GriffinLimVocoder(n_iter=-1)
    else:
        with pytest.raises(RuntimeError, match="no CPU path"):
            griffinlim.GriffinLimVocoder()


def test_checker_round_trip():
    rs = np.random.RandomState(3)
    for T in (2, 3, 8, 67):
        x = rs.randn(2, 256 * T) + np.array([[0.3], [-0.2]])
        back = ck.istft(ck.stft(x))
        err = float((back - torch.from_numpy(x)).abs().max())
        print("checker ISTFT(STFT(x)) T=%d: max abs error %.3e" % (T, err))
        assert tuple(back.shape) == (2, 256 * T) and err <= 1e-12


def test_checker_ignores_the_imaginary_parts_of_the_real_bins():
    rs = np.random.RandomState(4)
    S = torch.from_numpy(rs.randn(1, NBIN, 5) + 1j * rs.randn(1, NBIN, 5))
    S2 = S.clone()
    S2[:, 0].imag.zero_()
    S2[:, 512].imag.zero_()
    assert float((ck.istft(S) - ck.istft(S2)).abs().max()) <= 1e-15
