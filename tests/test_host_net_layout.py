"""CPU-only: the stash and scratch layouts of the network passes, seen through mcvc_net_layout (pure host code), are pinned by digest.
tests/golden/net_layout.json holds the SHA-256 of the row stream per configuration; it was recorded from gen_stash / shift_stash /
disc_stash and the walks' literal strides as they stood BEFORE the stash became one table per network and the walks' tensors shaped
descriptors (the entry added on top of the untouched code: `python tests/test_host_net_layout.py --record`), so equal digests say that
every offset, size, shape, stride, window shift and workspace need came out of the tables as it did out of the hand-written code.
Independent of the digests, the rows must tile the stash / the scratch up to the slabs, and a shifted window must stay inside its row."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

from mask_cyclegan_vc import _hip

MCVC_ERR_INVALID, MCVC_ERR_WORKSPACE = 1001, 1002
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "net_layout.json")
W = 12
GEN_SHAPES = [(1, 64), (2, 64), (3, 64), (8, 64), (32, 64), (1, 32), (2, 72), (1, 66), (2, 36), (1, 20)]
GEN_WINDOWS = [(1, 3, 1), (1, 3, 2), (2, 4, 2), (4, 6, 2), (2, 3, 0)]           # (B, stash_B, stash_b0), at T = 64 and T = 32
DISC_SHAPES = [(1, 64), (32, 64), (2, 68), (1, 66)]                             # (the last two: odd planes -> the dense sizes)


def layout(net, B, T, stash_B=0, b0=0):
    L = _hip.lib()
    n = ctypes.c_int(0)
    assert L.mcvc_net_layout(net, B, T, stash_B, b0, None, 0, ctypes.byref(n)) == MCVC_ERR_WORKSPACE
    rows = np.full((n.value, W), -1, dtype=np.int64)
    assert L.mcvc_net_layout(net, B, T, stash_B, b0, rows.ctypes.data, n.value, ctypes.byref(n)) == 0
    assert n.value == rows.shape[0]
    return rows


def configs():
    for B, T in GEN_SHAPES:
        yield (0, B, T, 0, 0)
    for T in (64, 32):
        for B, SB, b0 in GEN_WINDOWS:
            yield (0, B, T, SB, b0)
    for B, T in DISC_SHAPES:
        yield (1, B, T, 0, 0)


def record():
    return {"/".join(map(str, c)): hashlib.sha256(np.ascontiguousarray(layout(*c)).tobytes()).hexdigest() for c in configs()}


def test_every_layout_reproduces_its_recorded_digest():
    gold = json.load(open(GOLDEN))
    now = record()
    assert set(now) == set(gold)
    bad = [k for k in gold if now[k] != gold[k]]
    assert not bad, bad


def test_rows_tile_the_buffers_and_windows_stay_inside_their_rows():
    L = _hip.lib()
    for net, B, T, SB, b0 in configs():
        rows = layout(net, B, T, SB, b0)
        SB = max(SB, B)
        assert (rows[:-1, 0] > 0).all() and rows[-1, 0] == 3 and (rows[:-1, 1] == np.arange(len(rows) - 1)).all()
        stash_end = (L.mcvc_gen_stash_floats if net == 0 else L.mcvc_disc_stash_floats)(SB, T)
        for kind, end in ((1, stash_end), (2, int(rows[-1, 6]))):
            r = rows[rows[:, 0] == kind]
            off, floats = r[:, 2], r[:, 3]
            assert len(r) and (off % 4 == 0).all() and off[0] == 0 and (floats >= 0).all()
            assert (off[1:] == off[:-1] + ((floats[:-1] + 3) & ~3)).all()           # no gap, no overlap
            assert off[-1] + ((floats[-1] + 3) & ~3) == end
            # the last element the pass addresses from the window's first sample lies inside the row
            N, C, H, Wd, sb, sc, sh, win = (r[:, i] for i in range(4, 12))
            typed = N > 0
            last = win + (N - 1) * sb + (C - 1) * sc + (H - 1) * sh + (Wd - 1)
            assert (win[typed] >= off[typed]).all() and (last[typed & (C > 0)] < (off + floats)[typed & (C > 0)]).all()
            assert (win[~typed] == off[~typed]).all()
        assert (rows[-1, 2:6] >= 0).all() and (rows[-1, 2:6] % 4 == 0).all()
        scratch = (L.mcvc_gen_scratch_floats if net == 0 else L.mcvc_disc_scratch_floats)(B, T)
        assert scratch == rows[-1, 2:7].sum() + 64


def test_a_window_moves_batch_major_tensors_by_samples_and_trunk_tensors_by_rows():
    full = layout(0, 4, 64, 6, 0)
    win = layout(0, 4, 64, 6, 2)
    assert (full[:, :11] == win[:, :11]).all()
    st = full[:, 0] == 1
    moved = win[st, 11] - full[st, 11]
    assert (moved == 2 * full[st, 8]).all()            # b0 x the sample stride: per-sample floats, or W4 for [C][stash_B][W4]
    assert (full[st, 11] == full[st, 2]).all() and (win[~st, 11] == full[~st, 11]).all()


def test_invalid_arguments_are_refused():
    L = _hip.lib()
    n = ctypes.c_int(0)
    buf = np.zeros((4, W), dtype=np.int64)
    for args in [(2, 1, 64, 0, 0), (-1, 1, 64, 0, 0), (0, 0, 64, 0, 0), (0, 1, 0, 0, 0), (0, 1, 4, 0, 0), (0, 2, 64, 3, 2), (0, 1, 64, 3, -1),
                 (0, 1, 20, 3, 1), (1, 1, 64, 2, 0), (1, 1, 64, 0, 1)]:
        assert L.mcvc_net_layout(*args, None, 0, ctypes.byref(n)) == MCVC_ERR_INVALID, args
    assert L.mcvc_net_layout(0, 1, 64, 0, 0, None, 0, None) == MCVC_ERR_INVALID
    assert L.mcvc_net_layout(0, 1, 64, 0, 0, None, 4, ctypes.byref(n)) == MCVC_ERR_INVALID
    assert L.mcvc_net_layout(0, 1, 64, 0, 0, buf.ctypes.data, 4, ctypes.byref(n)) == MCVC_ERR_WORKSPACE and n.value > 4


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        json.dump(record(), open(GOLDEN, "w"), indent=1, sort_keys=True)
        print("wrote", GOLDEN)
