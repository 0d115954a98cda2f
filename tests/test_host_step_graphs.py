"""The training step's task graphs (mask_cyclegan_vc/step_graphs.py) are data: checked here without a GPU.

For every combination of every graph function's flags: list order is a valid one-stream order (serial mode runs it as it stands), event
names are unique, lanes are the four the engine has, and every part is one the engine's builders declare.  The graphs of the
configurations the benchmark and the default trainer run are pinned as literal tables (lanes and edges; the GPU tests pin what the
parts compute)."""
import itertools

import pytest

from mask_cyclegan_vc import step_graphs as sg

G, D = sg.G_PARTS[False], sg.D_PARTS[False]
GL, DL = sg.G_PARTS[True], sg.D_PARTS[True]


def _bools(n):
    return list(itertools.product((False, True), repeat=n))


# (graph function, its arguments, the part names it may use)
CASES = [(sg.four_lane_g, a, GL) for a in _bools(2)] \
    + [(sg.four_lane_d, a, DL) for a in _bools(2)] \
    + [(sg.grouped_g, a + (ln,), G) for a in _bools(2) for ln in ((1, 1), (2, 3))] \
    + [(sg.grouped_d, a, D) for a in _bools(1)] \
    + [(sg.pipelined, a, G | D) for a in _bools(5)] \
    + [(sg.merged, a, G | D) for a in _bools(3)] \
    + [(sg.ranged_update, (w,), G) for w in ((), ("cyc",))]


@pytest.mark.parametrize("fn,args,names", CASES, ids=["%s%s" % (f.__name__, a) for f, a, _ in CASES])
def test_graph_is_well_formed(fn, args, names):
    tasks = fn(*args)
    recorded, parts = set(), set()
    outer = set(args[0]) if fn is sg.ranged_update else set()       # (the helper's waits name events of the graph it is spliced into)
    for lane, part, waits, record in tasks:
        assert lane in (0, 1, 2, 3)
        assert isinstance(part, str) and part in names, part
        assert part not in parts, "part %s appears twice" % part
        parts.add(part)
        for w in waits:
            assert w in recorded or w in outer, "%s waits for %s, which no earlier task records" % (part, w)
        if record is not None:
            assert record not in recorded, "event %s recorded twice" % record
            recorded.add(record)


def test_part_name_sets_and_final_events():
    assert not (G & D) and not (GL & DL)                             # a pipelined graph resolves its names in both phases' parts
    for fin, graph in ((sg.FINAL_GROUPED, sg.grouped_g(True, True)), (sg.FINAL_LANED, sg.four_lane_g(True, True)),
                       (sg.FINAL_GROUPED, sg.pipelined(False, False, True, True, True)), (sg.FINAL_GROUPED, sg.merged(True, True, True))):
        recorded = {t[3] for t in graph}
        assert len(fin) == 2 and set(fin) <= recorded               # the events the gradient exchange of the last range waits for exist


# ---- the graphs of the benchmark (bs=1: pipelined; bs=8, 32: four lanes, split halves) and of the default trainer, as tables ----------
def test_pipelined_default_graph():
    assert sg.pipelined(split=False, serial=False, ranged=True, ov=False, tail=True) == [
        (1, "gen_fwd", (), "gen"),
        (0, "fwd", (), "g"),
        (1, "d_cycles", (), "cyc"),
        (0, "cycle", (), None),
        (3, "full1", ("gen",), None),
        (3, "dupd1", (), "dupd1"),
        (1, "full2", (), None),
        (1, "dupd2", (), "dupd2"),
        (2, "adv1", ("g", "dupd1"), "d1"),
        (2, "d_post_publish", ("dupd2",), None),
        (0, "adv2", ("dupd2",), None),
        (0, "bwd_cycle", ("d1",), None),
        (0, "bwd_final", (), "f"),
        (2, "g_post", ("f",), None),
        (1, "update_range0", ("cyc",), None),
        (1, "update_range1", (), None),
        (1, "update_range2", (), None),
        (1, "update_range3", (), None),
        (0, "update_range4", ("cyc",), None),
    ]


def test_pipelined_first_iteration_graph():
    assert sg.grouped_g(True, False, lanes=(2, 3)) == [
        (0, "fwd", (), "g"),
        (0, "cycle", (), None),
        (2, "adv1", ("g",), "d1"),
        (0, "adv2", (), None),
        (0, "bwd_cycle", ("d1",), None),
        (0, "bwd_final", (), "f"),
        (0, "update", (), None),
    ]
    assert sg.grouped_g(True, True, lanes=(2, 3))[6:] == [(3, "queue_reduce", (), None), (0, "update", (), None)]


def test_four_lane_generator_graph():
    assert sg.four_lane_g(True, False) == [
        (0, "fwd_A", (), "g0"),
        (1, "fwd_B", (), "g1"),
        (0, "cycle_A", (), None),
        (1, "cycle_B", (), None),
        (2, "finish_d", (), None),
        (2, "adv1_A", ("g1",), "dA"),
        (3, "adv1_B", ("g0",), "dB"),
        (0, "adv2_A", (), None),
        (1, "adv2_B", (), None),
        (0, "bwd_cycle_A", ("dB",), "c0"),
        (1, "bwd_cycle_B", ("dA",), "c1"),
        (0, "bwd_final_A", ("c1",), "fA2B"),
        (1, "bwd_final_B", ("c0",), "fB2A"),
        (0, "update_A", (), None),
        (1, "update_B", (), None),
    ]


def test_four_lane_discriminator_graphs():
    assert sg.four_lane_d(packed=True, split=True) == [
        (0, "gen_fwd_A", (), "gB"),
        (1, "gen_fwd_B", (), "gA"),
        (2, "refresh", (), None),
        (2, "real1_A", (), None),
        (3, "real1_B", (), None),
        (2, "real2_A", (), "rA2"),
        (3, "real2_B", (), "rB2"),
        (0, "d_cycles_A", (), None),
        (1, "d_cycles_B", (), None),
        (2, "fake1_A", ("gA",), None),
        (3, "fake1_B", ("gB",), None),
        (0, "fake2_A", ("rA2",), None),
        (1, "fake2_B", ("rB2",), None),
    ]
    assert sg.four_lane_d(True, False) == [
        (0, "gen_fwd_A", (), "gB"),
        (1, "gen_fwd_B", (), "gA"),
        (2, "refresh", (), None),
        (0, "d_cycles_A", (), None),
        (1, "d_cycles_B", (), None),
        (2, "full1_A", ("gA",), None),
        (3, "full1_B", ("gB",), None),
        (0, "full2_A", (), None),
        (1, "full2_B", (), None),
    ]


def test_grouped_discriminator_graph():
    assert sg.grouped_d(False) == [
        (0, "gen_fwd", (), "gen"),
        (1, "refresh", (), None),
        (0, "d_cycles", (), None),
        (1, "full1", ("gen",), None),
        (0, "full2", (), None),
    ]
