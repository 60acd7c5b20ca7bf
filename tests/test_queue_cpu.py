"""velocity_amd.driver.queue_plan: the schedule run_queue follows (no GPU).  Greedy and FIFO -- at every global step each free slot takes the next waiting
clip in (session, slot) order; a clip of n frames is admitted (frame 0) and tracked (frame 1) in its first step and holds its slot for n - 1 steps."""
import numpy as np
import pytest

from velocity_amd.driver import queue_plan

CASES = [([12, 4, 7, 9, 2, 12, 3], 3, 1), ([5], 3, 1), ([int(n) for n in np.random.default_rng(20240607).integers(2, 14, 20)], 4, 2)]


def _greedy_steps(lengths, streams):
    """The same rule, simulated without any notion of sessions or plans: a list of busy-until times."""
    free_at, t, nxt = [0] * streams, 0, 0   # free_at[s]: the first step at which slot s is free again
    last = 0
    while nxt < len(lengths):
        for s in range(streams):
            if free_at[s] <= t and nxt < len(lengths):
                free_at[s] = t + lengths[nxt] - 1
                last = max(last, free_at[s])
                nxt += 1
        t += 1
    return last


@pytest.mark.parametrize("lengths,streams,sessions", CASES)
def test_queue_plan_is_greedy_fifo_and_gapless(lengths, streams, sessions):
    plan = queue_plan(lengths, streams, sessions)
    sizes = [len(row) for row in plan[0]["frames"]]
    assert len(sizes) == min(sessions, streams) and sum(sizes) == streams and max(sizes) - min(sizes) <= 1
    # every clip is admitted exactly once, in FIFO order, in (session, slot) order within a step
    admitted = [a for st in plan for a in st["admit"]]
    assert [k for _, _, k in admitted] == list(range(len(lengths)))
    for st in plan:
        assert [(g, j) for g, j, _ in st["admit"]] == sorted((g, j) for g, j, _ in st["admit"])
    # a clip's frames 1 .. n-1 sit on consecutive steps of the slot it was admitted into, starting at its admission step; it is done at its last one
    seen = {}
    for t, st in enumerate(plan):
        held = [e for row in st["frames"] for e in row if e is not None]
        assert len({k for k, _ in held}) == len(held), "a clip in two slots"   # (a slot holds one entry by construction: no slot holds two clips)
        for g, row in enumerate(st["frames"]):
            for j, e in enumerate(row):
                if e is not None:
                    seen.setdefault(e[0], []).append((t, g, j, e[1]))
    t_admit = {k: t for t, st in enumerate(plan) for _, _, k in st["admit"]}
    t_done = {k: t for t, st in enumerate(plan) for _, _, k in st["done"]}
    slot_of = {k: (g, j) for g, j, k in admitted}
    assert sorted(t_done) == list(range(len(lengths)))
    for k, n in enumerate(lengths):
        assert [(t, g, j, i) for t, g, j, i in seen[k]] == [(t_admit[k] + i - 1,) + slot_of[k] + (i,) for i in range(1, n)], k
        assert t_done[k] == t_admit[k] + n - 2
    # a freed slot is refilled at the very next step while clips wait: no slot is empty at a step at which a later clip has not yet been admitted
    for t, st in enumerate(plan):
        waiting = sum(1 for k in range(len(lengths)) if t_admit[k] > t)
        if waiting:
            assert all(e is not None for row in st["frames"] for e in row), t
    # as many steps as the greedy rule needs
    assert len(plan) == _greedy_steps(lengths, streams)


def test_queue_plan_rejects_a_clip_of_one_frame():
    with pytest.raises(ValueError):
        queue_plan([3, 1], 2, 1)
