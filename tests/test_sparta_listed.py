"""ListedPlan (gym_amd.strategy.sparta) on the CPU: the index lists of the two cycle
selectors against get_indices of a fresh selector of the same class run from the same
seed -- the same sets every step, the closed-form counts, skipped tensors left alone, and
the torch generator in the same state after every step."""
import math

import pytest
import torch

from gym_amd.arena import ArenaLayout
from gym_amd.strategy.sparta import ListedPlan, PartitionedIndexSelector, ShuffledSequentialIndexSelector

NUMELS = [3, 64, 65, 1, 200]  # 3 < parts: empty partitions (Shuffled); 1: parts = 1, drawn every step (Partitioned)
SKIPPED, SKIP_STEPS = 2, (3, 4)


@pytest.mark.parametrize("cls,p", [(ShuffledSequentialIndexSelector, 0.1), (PartitionedIndexSelector, 0.25)])
def test_plan_matches_get_indices(cls, p):
    L = ArenaLayout([(m,) for m in NUMELS])
    params = [torch.zeros(m) for m in NUMELS]
    parts = math.ceil(1.0 / p)
    plan, ref = ListedPlan(cls(p, listed=True), L, L.n, "cpu"), cls(p)
    gen_plan = gen_ref = torch.manual_seed(11).get_state()
    cycle = [0] * len(NUMELS)  # Partitioned: the steps each tensor has taken part in
    for it in range(2 * parts + 2):  # a Partitioned redraw and a ShuffledSequential wrap
        skip = {SKIPPED} if it in SKIP_STEPS else set()
        torch.set_rng_state(gen_ref)
        want = {i: ref.get_indices(prm, it).nonzero().flatten() for i, prm in enumerate(params) if i not in skip}
        gen_ref = torch.get_rng_state()
        torch.set_rng_state(gen_plan)
        cur = list(plan.cur)
        rows, total, _ = plan.step(params, skip, it)
        gen_plan = torch.get_rng_state()
        assert torch.equal(gen_plan, gen_ref), it
        assert plan.cur[SKIPPED] == cur[SKIPPED] or not skip  # a skipped tensor does not advance
        by_start = {start: count for start, count in rows}
        assert total == sum(by_start.values()) == sum(w.numel() for w in want.values())
        for i, m in enumerate(NUMELS):
            np_ = parts if cls is ShuffledSequentialIndexSelector else max(1, min(parts, m))
            c = it % np_ if cls is ShuffledSequentialIndexSelector else cycle[i] % np_
            size, rem = divmod(m, np_)
            start, count = L.offsets[i] + c * size + min(c, rem), size + (c < rem)
            if i in skip:  # no row (len(rows) below) and no advance
                continue
            cycle[i] += 1
            assert by_start.get(start, 0) == count == want[i].numel(), (it, i)
            got = plan.order[start:start + count].long() - L.offsets[i]
            assert torch.equal(got.sort().values, want[i]), (it, i)
        assert len(rows) == sum(1 for i in want if want[i].numel())
        tab = plan.table(rows)
        assert tab.dtype == torch.int32 and tab[:, 1].sum() == total
        assert torch.equal(tab[:, 2], tab[:, 1].cumsum(0, dtype=torch.int32) - tab[:, 1])
