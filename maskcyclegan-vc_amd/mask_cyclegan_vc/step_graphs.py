"""The task graphs of the training step as data (no torch, no HIP: a graph can be read and tested without a GPU).

A graph is a list of ``(lane, part_name, waits, record)`` in a valid one-stream order: ``engine._run_tasks`` queues the part of that
name on lane ``lane``'s stream (lane 0 = the caller's) after the events named in ``waits`` and records the event ``record`` behind it.
The parts are built once per phase by ``engine._g_parts`` / ``engine._d_parts``; a part with an A- and a B-direction goes out either
GROUPED (one task ``name`` that runs both directions as one set of grouped launches) or LANED (two tasks ``name_A`` / ``name_B`` on
two lanes).  The four schedules are graphs over those parts:

    four_lane_g / four_lane_d     more than ``grouped_max_b`` samples per pass
    grouped_g / grouped_d         grouped launches, the two phases back to back (``flush()``, tests)
    pipelined                     grouped; iteration t's discriminator phase beside iteration t+1's generator phase (default)
    merged                        ... with the discriminator phase's generator forwards inside the generator phase's passes
"""

# event behind the last backward pass over each generator (A2B, B2A): the gradient exchange of the last parameter range waits for it
FINAL_GROUPED = ("f", "f")
FINAL_LANED = ("fA2B", "fB2A")

_G_PAIRS = ("fwd", "cycle", "adv1", "adv2", "bwd_cycle", "bwd_final")
_D_PAIRS = ("gen_fwd", "d_cycles", "repack", "full1", "full2", "real1", "real2", "fake1", "fake2")
_UPDATE_RANGES = tuple("update_range%d" % k for k in range(5))


def _laned(names):
    return [n + d for n in names for d in ("_A", "_B")]


# the names each builder must provide: {laned: names}
G_PARTS = {False: frozenset(_G_PAIRS + _UPDATE_RANGES + ("queue_reduce", "update", "g_post")),
           True: frozenset(_laned(_G_PAIRS + ("update",)) + ["finish_d", "queue_reduce"])}
D_PARTS = {False: frozenset(_D_PAIRS + ("refresh", "dupd1", "dupd2", "d_post_publish")),
           True: frozenset(_laned(_D_PAIRS) + ["refresh"])}


def four_lane_g(fuse_update, ov):
    """Generator phase on four lanes.  Lane 0 follows real_A -> fake_B -> cycle_A -> D_A2 and back, lane 1 follows real_B -> fake_A ->
    cycle_B -> D_B2 and back: these two are the critical path.  The first-step adversarial terms D_A(fake_A), D_B(fake_B) need only the
    translated batches: lanes 2 and 3 run their forward, loss and data-gradient WHILE lanes 0/1 are in the cycle forwards.  Cross-lane
    edges: the translated batches (g0, g1), the adversarial gradients that the cycle backward accumulates onto (dA, dB), and the two
    backward passes of one generator, which accumulate into the same weight gradients (c0, c1).  ``fuse_update``: each lane also runs
    the optimizer step of the generator whose last backward pass it ran (no join of the lanes)."""
    fA, fB = FINAL_LANED
    return [
        (0, "fwd_A", (), "g0"),
        (1, "fwd_B", (), "g1"),
        (0, "cycle_A", (), None),
        (1, "cycle_B", (), None),
        (2, "finish_d", (), None),             # (lane 2 is the first to need the discriminators)
        (2, "adv1_A", ("g1",), "dA"),
        (3, "adv1_B", ("g0",), "dB"),
        (0, "adv2_A", (), None),
        (1, "adv2_B", (), None),
        # backward through the cycle passes: cycle_A = G_B2A(fake_B) adds to d(fake_B), cycle_B = G_A2B(fake_A) to d(fake_A)
        (0, "bwd_cycle_A", ("dB",), "c0"),
        (1, "bwd_cycle_B", ("dA",), "c1"),
        # the last pass over each generator
        (0, "bwd_final_A", ("c1",), fA),
        (1, "bwd_final_B", ("c0",), fB),
    ] + ([(2, "queue_reduce", (), None)] if (fuse_update and ov) else []) \
      + ([(0, "update_A", (), None), (1, "update_B", (), None)] if fuse_update else [])


def four_lane_d(packed, split):
    """Discriminator phase on four lanes.  Same shape as the generator phase: lanes 0/1 carry the two generator chains, D_A / D_B need
    only the generated batches and run on lanes 2/3 while lanes 0/1 are in the cycle forwards; the second-step discriminators follow
    the cycle forwards on lanes 0/1.  ``packed``: the generator phase left lane 0 with generator_A2B updated and its copies fresh, lane
    1 with generator_B2A, so each lane starts with its own generator.  ``split``: the real halves need nothing from the generators:
    lanes 2/3 run them while lanes 0/1 are in the generator forwards, so the tail of the phase (second-step discriminators behind the
    cycle forwards) is a pass over the generated half only.  A discriminator's two passes add into the same gradients: same lane, or
    ordered by an event."""
    if not packed:
        # (phase called on its own: a lane re-packs the generator it runs first; the other lane's second pass waits for that re-pack)
        return [
            (0, "repack_B", (), "p0"),
            (1, "repack_A", (), "p1"),
            (0, "gen_fwd_B", (), "gA"),
            (1, "gen_fwd_A", (), "gB"),
            (0, "d_cycles_B", ("p1",), None),
            (1, "d_cycles_A", ("p0",), None),
            (2, "full1_A", ("gA",), None),
            (3, "full1_B", ("gB",), None),
            (0, "full2_B", (), None),
            (1, "full2_A", (), None),
        ]
    head = [(0, "gen_fwd_A", (), "gB"), (1, "gen_fwd_B", (), "gA"), (2, "refresh", (), None)]
    cycles = [(0, "d_cycles_A", (), None), (1, "d_cycles_B", (), None)]
    if split:
        return head + [
            (2, "real1_A", (), None),
            (3, "real1_B", (), None),
            (2, "real2_A", (), "rA2"),
            (3, "real2_B", (), "rB2"),
        ] + cycles + [
            (2, "fake1_A", ("gA",), None),
            (3, "fake1_B", ("gB",), None),
            (0, "fake2_A", ("rA2",), None),
            (1, "fake2_B", ("rB2",), None),
        ]
    return head + cycles + [
        (2, "full1_A", ("gA",), None),
        (3, "full1_B", ("gB",), None),
        (0, "full2_A", (), None),
        (1, "full2_B", (), None),
    ]


def grouped_g(fuse_update, ov, lanes=(1, 1)):
    """Generator phase in grouped launches: the dataflow of ``four_lane_g`` on two lanes.  Lane 0: both translation (+ identity)
    passes, both cycle passes, the second-step discriminators, both backward rounds, the update.  ``lanes`` = (lane of the first-step
    adversarial pair D_A(fake_A) | D_B(fake_B), which needs only the translated batches and runs beside the cycle forwards; lane of
    the gradient exchange): (1, 1) for the phase on its own, (2, 3) for the first iteration of the pipelined step."""
    adv, red = lanes
    return [
        (0, "fwd", (), "g"),
        (0, "cycle", (), None),
        (adv, "adv1", ("g",), "d1"),
        (0, "adv2", (), None),
        (0, "bwd_cycle", ("d1",), None),
        (0, "bwd_final", (), FINAL_GROUPED[0]),
    ] + ([(red, "queue_reduce", (), None)] if (fuse_update and ov) else []) \
      + ([(0, "update", (), None)] if fuse_update else [])


def grouped_d(split):
    """Discriminator phase in grouped launches: lane 0 runs both generators' forwards (translation, then cycle) and the second-step
    discriminator pair, lane 1 runs D_A | D_B.  ``refresh`` clears the generator gradients beside the generator forwards."""
    if split:
        # the real halves need nothing from the generators: lane 1 runs them while lane 0 is in the generator forwards
        return [
            (0, "gen_fwd", (), "gen"),
            (1, "refresh", (), None),
            (1, "real1", (), None),
            (1, "real2", (), "r2"),
            (0, "d_cycles", (), None),
            (1, "fake1", ("gen",), None),
            (0, "fake2", ("r2",), None),
        ]
    return [
        (0, "gen_fwd", (), "gen"),
        (1, "refresh", (), None),
        (0, "d_cycles", (), None),
        (1, "full1", ("gen",), None),
        (0, "full2", (), None),
    ]


def ranged_update(waits):
    """The generator update range by range: the up-sampling blocks', the trunk's and most of the head's optimizer step + re-pack run on
    lane 1 beside the rest of the last backward pass, behind its milestone events (and ``waits``: everything that still reads the old
    weights); only conv1's is left for the end of the chain."""
    return [(1, "update_range0", waits, None), (1, "update_range1", (), None), (1, "update_range2", (), None),
            (1, "update_range3", (), None), (0, "update_range4", waits, None)]


def pipelined(split, serial, ranged, ov, tail):
    """Iteration t+1's generator phase beside iteration t's discriminator phase, as ONE graph:
        lane 1:  D-phase(t): generator forwards -> cycle forwards -> D_A2 | D_B2 -> [all-reduce] update of their slice -> "dupd2";
                 then the ranged generator update of G-phase(t+1) behind the last backward pass's milestone events (idle since "dupd2")
        lane 3:  D_A | D_B of D-phase(t) -> update of their slice -> "dupd1"; the backward rounds' weight gradients (its stream)
        lane 0:  G-phase(t+1): translation (+ identity) -> cycle -> (dupd2) D_A2 | D_B2 adversarial -> backward x 2 -> conv1's update
        lane 2:  (dupd1) the first-step adversarial pair of G-phase(t+1)
    ``serial`` (data-parallel ranks): the G-phase's grouped forwards wait for the D-phase's generator forwards, one grouped persistent
    trunk pass in flight at a time.  ``tail``: the loss sums and the publish of iteration t's losses ride on lane 2 instead of the end
    of the chain.  The generator update waits for everything that still reads the old weights (D-phase(t)'s generator forwards: "cyc")."""
    tasks = [(1, "gen_fwd", (), "gen")] + ([(1, "d_cycles", (), "cyc")] if serial else []) + [
        (0, "fwd", ("cyc",) if serial else (), "g"),
    ]
    if split:
        tasks += [(3, "real1", (), None), (3, "real2", (), "r2")]
    tasks += ([] if serial else [(1, "d_cycles", (), "cyc")]) + [
        (0, "cycle", (), None),
        (3, "fake1" if split else "full1", ("gen",), None),
        (3, "dupd1", (), "dupd1"),
        (1, "fake2" if split else "full2", ("r2",) if split else (), None),
        (1, "dupd2", (), "dupd2"),
        (2, "adv1", ("g", "dupd1"), "d1"),
    ] + ([(2, "d_post_publish", ("dupd2",), None)] if tail else []) + [
        (0, "adv2", ("dupd2",), None),
        (0, "bwd_cycle", ("d1",), None),
        (0, "bwd_final", (), FINAL_GROUPED[0]),
    ] + ([(2, "g_post", (FINAL_GROUPED[0],), None)] if tail else []) + ([(3, "queue_reduce", (), None)] if ov else [])
    return tasks + (ranged_update(("cyc",)) if ranged else [(0, "update", ("cyc",), None)])


def merged(have_prev, ranged, ov):
    """``pipelined`` with the discriminator phase's generator forwards inside the generator phase's passes:
        lane 0: forward x3 -> cycle x2 -> the two backward passes -> conv1's update;  lanes 1 / 2: D_A | D_B (D_A2 | D_B2) of D-phase(t)
        -> their update -> first- (second-) step adversarial pair of G-phase(t+1), lane 1 then the ranged generator update;  lane 3:
        weight gradients (its stream) and the gradient exchange"""
    tasks = [(0, "fwd", (), "g"), (0, "cycle", (), "c")]
    if have_prev:
        tasks += [(1, "full1", ("g",), None), (1, "dupd1", (), None), (2, "full2", ("c",), None), (2, "dupd2", (), None)]
    tasks += [(1, "adv1", ("g",), "d1"), (2, "adv2", ("c",), "d2"),
              (0, "bwd_cycle", ("d1", "d2"), None), (0, "bwd_final", (), FINAL_GROUPED[0])]
    if ov:
        tasks += [(3, "queue_reduce", (), None)]
    return tasks + (ranged_update(()) if ranged else [(0, "update", (), None)])
