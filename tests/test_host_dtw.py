"""CPU-only checks of the objective-evaluation host side (mask_cyclegan_vc/metrics.py, the mcvc_dtw_* / mcvc_cep_* C ABI, the evaluate
parser) and of the float64 checker itself (tests/dtw_checker.py).  No kernel is launched here."""
import ctypes

import numpy as np
import pytest
import torch

import dtw_checker as ck
from args.evaluate_arg_parser import EvaluateArgParser
from mask_cyclegan_vc import _hip, metrics

MCVC_ERR_INVALID, MCVC_ERR_WORKSPACE = 1001, 1002
DTW_SYMBOLS = ("mcvc_dtw_max_frames", "mcvc_dtw_launches", "mcvc_cep_basis_init", "mcvc_cep_project", "mcvc_dtw_plan", "mcvc_dtw_run")


def offs_of(lengths):
    o = np.zeros(len(lengths) + 1, dtype=np.int32)
    np.cumsum(lengths, out=o[1:])
    return o


def plan(xl, yl, want_path, x_offs=None, y_offs=None, n=None):
    L = _hip.lib()
    xo = offs_of(xl) if x_offs is None else np.asarray(x_offs, dtype=np.int32)
    yo = offs_of(yl) if y_offs is None else np.asarray(y_offs, dtype=np.int32)
    n = xo.size - 1 if n is None else n
    table = np.zeros((max(n, 1), 6), dtype=np.int64)
    ws, rows = ctypes.c_longlong(-7), ctypes.c_longlong(-7)
    rc = L.mcvc_dtw_plan(xo.ctypes.data, yo.ctypes.data, n, want_path, table.ctypes.data, ctypes.byref(ws), ctypes.byref(rows))
    return rc, table, ws.value, rows.value


# ---- the checker against facts that need no kernel ------------------------------------------------------------------------------------
def test_checker_self_alignment_is_the_diagonal():
    rs = np.random.RandomState(0)
    for K, T in ((1, 1), (3, 7), (24, 65)):
        x = rs.randn(K, T)
        cost, length, path = ck.dtw(x, x)
        assert cost == 0.0 and length == T
        assert np.array_equal(path, np.stack([np.arange(T)] * 2, axis=1))


def test_checker_doubled_frames_cost_nothing():
    rs = np.random.RandomState(1)
    x = rs.randn(5, 9)
    cost, length, path = ck.dtw(x, np.repeat(x, 2, axis=1))
    assert cost == 0.0 and length == 18 and ck.path_is_valid(path, 9, 18)
    cost, length, path = ck.dtw(np.repeat(x, 2, axis=1), x)
    assert cost == 0.0 and length == 18 and ck.path_is_valid(path, 18, 9)


def test_checker_hand_worked_3_by_4():
    """x = (0, 2, 3), y = (0, 1, 2, 4), K = 1: d = |x_i - y_j|.  Worked by hand; ties at (1, 2) [diag = left] and (2, 2) [diag = up] go to the
    diagonal, because a later candidate replaces only on strict <."""
    x, y = np.array([[0.0, 2.0, 3.0]]), np.array([[0.0, 1.0, 2.0, 4.0]])
    cost, length, path, acc, ln, choice = ck.dtw(x, y, return_tables=True)
    assert np.array_equal(ck.frame_distances(x, y), [[0, 1, 2, 4], [2, 1, 0, 2], [3, 2, 1, 1]])
    assert np.array_equal(acc, [[0, 1, 3, 7], [2, 1, 1, 3], [5, 3, 2, 2]])
    assert np.array_equal(ln, [[1, 2, 3, 4], [2, 2, 3, 4], [3, 3, 3, 4]])
    assert choice[1, 2] == 0 and choice[2, 2] == 0 and choice[2, 1] == 1 and choice[1, 3] == 2
    assert cost == 2.0 and length == 4
    assert path.tolist() == [[0, 0], [0, 1], [1, 2], [2, 3]]
    assert ck.path_cost(x, y, path) == cost
    assert ck.dtw(x, y, scale=2.5)[0] == 5.0


def test_checker_single_frame_sides_give_straight_paths():
    rs = np.random.RandomState(2)
    x, y = rs.randn(4, 1), rs.randn(4, 6)
    cost, length, path = ck.dtw(x, y)
    assert length == 6 and path.tolist() == [[0, j] for j in range(6)]
    assert abs(cost - ck.frame_distances(x, y).sum()) <= 1e-12
    cost, length, path = ck.dtw(y, x)
    assert length == 6 and path.tolist() == [[i, 0] for i in range(6)]
    assert abs(cost - ck.frame_distances(x, y).sum()) <= 1e-12
    assert ck.dtw(x, x)[:2] == (0.0, 1) and ck.dtw(x, x)[2].tolist() == [[0, 0]]


# ---- the constant operand -------------------------------------------------------------------------------------------------------------
def test_dct_basis_is_orthonormal_and_the_table_is_its_rounding():
    B = ck.full_dct()
    assert np.abs(B @ B.T - np.eye(80)).max() <= 1e-12
    assert np.abs(metrics.dct_basis(79) - B[1:]).max() <= 1e-15
    for n_cep in (1, 24, 79):
        host = metrics.host_basis(n_cep)
        assert host.shape == (n_cep, 80) and host.dtype == np.float32
        want = B[1:n_cep + 1]
        err = float(np.abs(host.astype(np.float64) - want).max())
        print("n_cep %d: float32 table against the float64 basis, max abs difference %.3e" % (n_cep, err))
        assert err <= 2.0 ** -24 * np.abs(want).max() * 1.01 + 1e-16          # one rounding (cos of two libraries: a few 1e-17)
        assert np.count_nonzero(host != want.astype(np.float32)) <= 1 + host.size // 100
    L = _hip.lib()
    buf = np.zeros(80 * 80, dtype=np.float32)
    for bad in (0, 80, -1):
        assert L.mcvc_cep_basis_init(bad, buf.ctypes.data) == MCVC_ERR_INVALID
    assert L.mcvc_cep_basis_init(24, None) == MCVC_ERR_INVALID
    for bad in (0, 80):
        with pytest.raises(ValueError):
            metrics.host_basis(bad)


def test_symbols_are_bound():
    L = _hip.lib()
    for name in DTW_SYMBOLS:
        assert name in _hip.EXPORTED_SYMBOLS and getattr(L, name).argtypes is not None
    assert L.mcvc_version() == 3
    assert L.mcvc_dtw_max_frames() >= 4096 and metrics.max_frames() == L.mcvc_dtw_max_frames()
    assert L.mcvc_dtw_launches(0) == 1 and L.mcvc_dtw_launches(1) == 2


# ---- plan and limits --------------------------------------------------------------------------------------------------------------------
def test_plan_refuses_bad_tables():
    M = _hip.lib().mcvc_dtw_max_frames()
    assert plan([3, 4], [5, 6], 1)[0] == 0
    assert plan(None, [5, 6], 1, x_offs=[0, 5, 3])[0] == MCVC_ERR_INVALID             # not monotone
    assert plan([3, 4], None, 1, y_offs=[0, 6, 6])[0] == MCVC_ERR_INVALID             # an utterance of no frames
    assert plan([0, 4], [5, 6], 0)[0] == MCVC_ERR_INVALID
    assert plan([3, M + 1], [5, 6], 0)[0] == MCVC_ERR_INVALID                         # over the limit
    assert plan([3, 4], [M + 1, 6], 1)[0] == MCVC_ERR_INVALID
    assert plan([3, M], [M, 6], 1)[0] == 0                                            # the limit itself is allowed
    assert plan([3, 4], [5, 6], 0, n=0)[0] == MCVC_ERR_INVALID                        # n_pairs = 0
    assert plan(None, [5, 6], 0, x_offs=[-1, 2, 5])[0] == MCVC_ERR_INVALID
    L = _hip.lib()
    ws, rows = ctypes.c_longlong(0), ctypes.c_longlong(0)
    o = offs_of([3, 4])
    assert L.mcvc_dtw_plan(None, o.ctypes.data, 2, 0, None, ctypes.byref(ws), ctypes.byref(rows)) == MCVC_ERR_INVALID
    assert L.mcvc_dtw_plan(o.ctypes.data, o.ctypes.data, 2, 0, None, None, ctypes.byref(rows)) == MCVC_ERR_INVALID
    assert L.mcvc_dtw_plan(o.ctypes.data, o.ctypes.data, 2, 1, None, ctypes.byref(ws), ctypes.byref(rows)) == 0 and ws.value > 0     # sizes only
    with pytest.raises(ValueError, match="refused"):
        metrics.plan(offs_of([3, M + 1]), offs_of([5, 6]), False)
    with pytest.raises(ValueError, match="same number"):
        metrics.plan(offs_of([3, 4]), offs_of([5]), False)


def test_plan_sizes_and_table():
    rc, table, ws0, rows0 = plan([70, 5, 200], [90, 1, 37], 0)
    assert rc == 0 and ws0 == 0 and rows0 == 0                                        # the default call: no Tx x Ty matrix, nothing at all
    assert table[:, :4].tolist() == [[0, 70, 0, 90], [70, 5, 90, 1], [75, 200, 91, 37]] and (table[:, 4:] == -1).all()
    rc, table, ws1, rows1 = plan([70, 5, 200], [90, 1, 37], 1)
    assert rc == 0 and rows1 == (70 + 90 - 1) + (5 + 1 - 1) + (200 + 37 - 1)
    assert ws1 >= 70 * 90 + 5 * 1 + 200 * 37                                          # one direction byte per cell at the least
    assert table[:, 5].tolist() == [0, 159, 164]
    assert table[0, 4] == 0 and (np.diff(table[:, 4]) > 0).all() and (table[:, 4] % 16 == 0).all()
    # each pair's direction bytes end where the next pair's begin, inside the workspace
    assert table[1, 4] - table[0, 4] >= 70 * 90 and table[2, 4] - table[1, 4] >= 5 and ws1 - table[2, 4] >= 200 * 37
    prev = 0
    for T in (1, 2, 63, 64, 65, 128, 129, 900):                                       # grows with the lengths
        cur = plan([T], [T], 1)[2]
        assert cur > prev and cur >= T * T
        prev = cur
    assert plan([64], [100], 1)[2] < plan([65], [100], 1)[2] and plan([64], [100], 1)[2] < plan([64], [101], 1)[2]


# ---- refusals before a launch -------------------------------------------------------------------------------------------------------------
def test_run_refuses_before_it_touches_a_device():
    """Every refusal comes from the argument check: the device pointers are never followed, no device is needed."""
    L = _hip.lib()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    xo, yo = offs_of([70, 5]), offs_of([90, 3])
    X, Y = int(xo[-1]), int(yo[-1])
    rc, _, ws, rows = plan([70, 5], [90, 3], 1)
    assert rc == 0 and ws > 0

    def run(x=p, y=p, K=24, scale=1.0, xo_=xo, yo_=yo, table=p, n=2, cost=p, length=p, path=p, w=p, wb=ws, xf=X, yf=Y):
        return L.mcvc_dtw_run(x, xf, y, yf, K, scale, xo_.ctypes.data, yo_.ctypes.data, table, n, cost, length, path, w, wb, None)

    for kw in (dict(x=None), dict(y=None), dict(table=None), dict(cost=None), dict(length=None)):           # null pointers
        assert run(**kw) == MCVC_ERR_INVALID, kw
    assert run(table=p + 8) == MCVC_ERR_INVALID                                       # the table off the 16-byte boundary
    assert run(x=p + 2) == MCVC_ERR_INVALID and run(cost=p + 1) == MCVC_ERR_INVALID and run(path=p + 2) == MCVC_ERR_INVALID
    assert run(w=p + 4) == MCVC_ERR_INVALID
    assert run(K=0) == MCVC_ERR_INVALID and run(K=81) == MCVC_ERR_INVALID and run(K=-3) == MCVC_ERR_INVALID
    assert run(n=0) == MCVC_ERR_INVALID
    assert run(scale=float("nan")) == MCVC_ERR_INVALID
    assert run(xf=X - 1) == MCVC_ERR_INVALID and run(yf=Y - 1) == MCVC_ERR_INVALID    # tables that reach beyond the banks
    assert run(xo_=np.array([0, 70, 70], dtype=np.int32)) == MCVC_ERR_INVALID         # what the plan refuses, refused again
    assert run(wb=ws - 1) == MCVC_ERR_WORKSPACE                                       # one byte short
    assert run(w=None) == MCVC_ERR_WORKSPACE
    assert run(path=None, w=None, wb=0, K=0) == MCVC_ERR_INVALID                      # (without paths there is no workspace to be short of)


def test_projection_refuses_before_it_touches_a_device():
    L = _hip.lib()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    assert L.mcvc_cep_project(None, 10, p, 24, p, None) == MCVC_ERR_INVALID
    assert L.mcvc_cep_project(p, 10, None, 24, p, None) == MCVC_ERR_INVALID
    assert L.mcvc_cep_project(p, 10, p, 24, None, None) == MCVC_ERR_INVALID
    assert L.mcvc_cep_project(p, 10, p + 4, 24, p, None) == MCVC_ERR_INVALID          # the basis off the 16-byte boundary
    assert L.mcvc_cep_project(p + 2, 10, p, 24, p, None) == MCVC_ERR_INVALID
    assert L.mcvc_cep_project(p, 0, p, 24, p, None) == MCVC_ERR_INVALID
    assert L.mcvc_cep_project(p, 10, p, 0, p, None) == MCVC_ERR_INVALID
    assert L.mcvc_cep_project(p, 10, p, 80, p, None) == MCVC_ERR_INVALID


# ---- parser and module ------------------------------------------------------------------------------------------------------------------
def test_evaluate_parser():
    p = EvaluateArgParser()
    d = p.parser.parse_args([])
    assert d.n_cep == 24 and d.converted_dir is None and d.target_speaker_id is None and d.target_wav_dir is None and d.source_speaker_id is None
    assert d.name == "debug" and d.preprocessed_data_dir == "vcc2018_training_preprocessed/"
    a = p.parse_args(["--target_speaker_id", "VCC2TF1"])
    assert a.target_speaker_id == "VCC2TF1" and a.target_wav_dir is None and a.n_cep == 24
    a = p.parse_args(["--target_wav_dir", "wavs", "--source_speaker_id", "VCC2SF3", "--n_cep", "13"])
    assert a.target_wav_dir == "wavs" and a.source_speaker_id == "VCC2SF3" and a.n_cep == 13
    for bad in ([], ["--target_speaker_id", "VCC2TF1", "--target_wav_dir", "wavs"], ["--target_speaker_id", "VCC2TF1", "--n_cep", "0"],
                ["--target_speaker_id", "VCC2TF1", "--n_cep", "80"], ["--target_wav_dir", "wavs", "--n_cep", "many"]):
        with pytest.raises(SystemExit):
            EvaluateArgParser().parse_args(bad)


def test_module_has_no_cpu_path_and_checks_its_input():
    x = [np.zeros((3, 4), dtype=np.float32)]
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            metrics.dtw(x, x)
        with pytest.raises(RuntimeError, match="no CPU path"):
            metrics.mel_cepstra([np.zeros((80, 4), dtype=np.float32)])
        with pytest.raises(RuntimeError, match="no CPU path"):
            metrics.mcd([np.zeros((80, 4), dtype=np.float32)], [np.zeros((80, 4), dtype=np.float32)])
    else:
        with pytest.raises(ValueError, match="finite"):
            metrics.dtw([np.full((3, 4), np.nan, dtype=np.float32)], x)
        with pytest.raises(ValueError):
            metrics.dtw(x, [np.zeros((2, 4), dtype=np.float32)])
        with pytest.raises(ValueError):
            metrics.dtw(x, x + x)
        with pytest.raises(ValueError):
            metrics.dtw([np.zeros((81, 4), dtype=np.float32)], [np.zeros((81, 4), dtype=np.float32)])
        with pytest.raises(ValueError):
            metrics.mel_cepstra([np.zeros((79, 4), dtype=np.float32)])
    with pytest.raises(ValueError):
        metrics.dct_basis(80)
