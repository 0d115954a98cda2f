"""CPU-only: the job tables of every restricted re-pack / fused update, seen through mcvc_pack_plan (pure host code), are pinned
by digest.  tests/golden/pack_plan.json holds the SHA-256 of the row stream per configuration; it was recorded from the table builders
as they stood BEFORE the packed forms became rows of one catalogue (the entry added on top of the untouched builders:
`python tests/test_host_packplan.py --record`), so equal digests say that every job, owner, data-gradient argument entry, byte count and
packed offset came out of the catalogue as it did out of the hand-written blocks."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from mask_cyclegan_vc import _hip

MCVC_ERR_INVALID, MCVC_ERR_WORKSPACE = 1001, 1002
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_plan.json")
W = 20
GEN_SHAPES = [(1, 64), (2, 64), (4, 64), (8, 64), (32, 64), (1, 32), (2, 72), (1, 256), (2, 66)]
RANGES = [7, 1, 2, 4, 8, 16, 32, 3, 56]
DISC_SHAPES = [(1, 64), (32, 64), (2, 68)]
FLAGS = ["fused", "wino_only", "w4", "w43", "up1_w4", "up1_w2", "up2_w2"]


def plan(net, mb, T, sets, rmask, update):
    L = _hip.lib()
    n = ctypes.c_int(0)
    assert L.mcvc_pack_plan(net, mb, T, sets, rmask, update, None, 0, ctypes.byref(n)) in (0, MCVC_ERR_WORKSPACE)
    rows = np.full((n.value, W), -1, dtype=np.int64)
    assert L.mcvc_pack_plan(net, mb, T, sets, rmask, update, rows.ctypes.data, n.value, ctypes.byref(n)) == 0
    assert n.value == rows.shape[0] and rows[0, 0] == 0 and rows[0, 11] == W
    return rows


def configs():
    for mb, T in GEN_SHAPES:
        for r in RANGES:
            for sets in (1, 2, 3):
                yield (0, mb, T, sets, r, 0)
            yield (0, mb, T, 3, r, 1)
    for mb, T in DISC_SHAPES:
        yield (1, mb, T, 3, 7, 0)
        yield (1, mb, T, 3, 7, 1)


def record():
    out = {"digests": {}, "gen_flags": {}, "disc_kind": {}}
    for c in configs():
        rows = plan(*c)
        out["digests"]["/".join(map(str, c))] = hashlib.sha256(np.ascontiguousarray(rows).tobytes()).hexdigest()
        if c[0] == 0:
            out["gen_flags"]["%d/%d" % c[1:3]] = {f: int(rows[0, 10]) >> i & 1 for i, f in enumerate(FLAGS)}
        else:
            out["disc_kind"]["%d/%d" % c[1:3]] = int(rows[0, 10])
    return out


def test_every_plan_reproduces_its_recorded_digest():
    gold = json.load(open(GOLDEN))
    now = record()
    assert set(now["digests"]) == set(gold["digests"])
    bad = [k for k in gold["digests"] if now["digests"][k] != gold["digests"][k]]
    assert not bad, bad
    assert now["gen_flags"] == gold["gen_flags"] and now["disc_kind"] == gold["disc_kind"]


def test_recorded_configurations_flip_every_planner_flag():
    gold = json.load(open(GOLDEN))
    for f in FLAGS:
        assert {v[f] for v in gold["gen_flags"].values()} == {0, 1}, f
    assert set(gold["disc_kind"].values()) == {1, 4} and gold["disc_kind"]["2/68"] == 1        # (T = 68: the fall-back to the full table)


def test_plan_is_consistent_with_itself():
    for c in [(0, 1, 64, 3, 7, 1), (0, 4, 64, 1, 3, 0), (1, 1, 64, 3, 7, 1), (1, 2, 68, 3, 7, 0)]:
        rows = plan(*c)
        hdr, jobs, own = rows[0], rows[rows[:, 0] == 1], rows[rows[:, 0] == 2]
        assert hdr[3] == len(jobs) and hdr[4] == len(own) and hdr[5] == (rows[:, 0] == 4).sum()
        assert (jobs[:, 5] >= 0).all() and (jobs[:, 6] > 0).all() and (jobs[:, 5] + jobs[:, 6] <= hdr[7]).all()     # regions inside the buffer
        assert ((jobs[:, 2] >= 0) & (jobs[:, 2] < 14)).all()
        fresh = {int(r[1]): int(r[3]) for r in rows[rows[:, 0] == 3]}
        for layer in set(jobs[:, 1].tolist()):       # a layer's fresh mask is exactly the forms of its jobs
            m = 0
            for f in jobs[jobs[:, 1] == layer][:, 2]:
                m |= 1 << int(f)
            assert fresh[layer] == m
        if c[5]:
            assert own[:, 10].sum() == len(jobs)           # every job is the emit of exactly one owner
            assert (own[:, 9] == np.concatenate([[0], np.cumsum(own[:, 10])[:-1]])).all()


def test_update_plan_sizes_are_the_models_parameter_sizes():
    from mask_cyclegan_vc.model import Discriminator, Generator
    for net, model in ((0, Generator()), (1, Discriminator())):
        numel = [p.numel() for p in model.parameters()]
        own = plan(net, 1, 64, 3, 7, 1)
        own = own[own[:, 0] == 2]
        for o in own:
            assert (o[4] if o[11] else o[4] * o[5] * o[6]) == numel[int(o[1])], o


def test_invalid_arguments_are_refused():
    L = _hip.lib()
    n = ctypes.c_int(0)
    buf = np.zeros((4, W), dtype=np.int64)
    ptrs = (ctypes.c_void_p * 128)(*([buf.ctypes.data] * 128))
    bad_masks = [0, -1, 64, 100] + [m for m in range(1, 64) if (m & 4) and (m & 56)]
    for m in bad_masks:
        assert L.mcvc_pack_plan(0, 1, 64, 3, m, 0, None, 0, ctypes.byref(n)) == MCVC_ERR_INVALID, m
        assert L.mcvc_pack_plan(0, 1, 64, 3, m, 1, None, 0, ctypes.byref(n)) == MCVC_ERR_INVALID, m
        # the entries themselves refuse before they touch a pointer or the device
        assert L.mcvc_gen_pack_ranges(None, None, 1, 64, 3, m, None) == MCVC_ERR_INVALID, m
        assert L.mcvc_gen_update_ranges(ptrs, buf.ctypes.data, buf.ctypes.data, 1, 64, m, None, None, None, None, None,
                                        0.0, 0.9, 0.999, 1e-8, 1, 1.0, 0, None) == MCVC_ERR_INVALID, m
    for m in range(1, 64):
        if not ((m & 4) and (m & 56)):
            assert L.mcvc_pack_plan(0, 1, 64, 3, m, 0, None, 0, ctypes.byref(n)) in (0, MCVC_ERR_WORKSPACE), m
    for sets in (0, 4, -1, 7):
        assert L.mcvc_pack_plan(0, 1, 64, sets, 7, 0, None, 0, ctypes.byref(n)) == MCVC_ERR_INVALID, sets
        assert L.mcvc_gen_pack_ranges(None, None, 1, 64, sets, 7, None) == MCVC_ERR_INVALID, sets
    for sets in (1, 2):
        assert L.mcvc_pack_plan(0, 1, 64, sets, 7, 1, None, 0, ctypes.byref(n)) == MCVC_ERR_INVALID       # an update refreshes both sides
    assert L.mcvc_pack_plan(2, 1, 64, 3, 7, 0, None, 0, ctypes.byref(n)) == MCVC_ERR_INVALID
    assert L.mcvc_pack_plan(0, 1, 64, 3, 7, 2, None, 0, ctypes.byref(n)) == MCVC_ERR_INVALID
    assert L.mcvc_pack_plan(0, 0, 64, 3, 7, 0, None, 0, ctypes.byref(n)) == MCVC_ERR_INVALID
    assert L.mcvc_pack_plan(0, 1, 64, 3, 7, 0, None, 0, None) == MCVC_ERR_INVALID
    assert L.mcvc_pack_plan(0, 1, 64, 3, 7, 0, None, 4, ctypes.byref(n)) == MCVC_ERR_INVALID
    assert L.mcvc_pack_plan(0, 1, 64, 3, 7, 0, buf.ctypes.data, 4, ctypes.byref(n)) == MCVC_ERR_WORKSPACE and n.value > 4


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        json.dump(record(), open(GOLDEN, "w"), indent=1, sort_keys=True)
        print("wrote", GOLDEN)
