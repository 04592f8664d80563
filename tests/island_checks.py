"""numpy oracle of the island outer step -- TEST INFRASTRUCTURE.

The contract of include/gym_amd.h (ga_diloco_outer_islands), one individually rounded
fp32 operation per line, on float32 arrays (numpy rounds every float32 operation once,
to nearest even); the outer update from the pseudo-gradient on is quant_checks'
outer_from_g, its fused multiply-adds fma32 (one rounding).  Beside it the host side,
stated independently: FedAvg's island draw (draw) and a replay of whole rounds over
given per-step row contents (run).
"""
import random

import numpy as np

from quant_checks import bf16_round, outer_from_g

f32 = np.float32


def _store(x, bf16):
    """The value an arena of the dtype holds after storing fp32 x."""
    x = np.asarray(x, f32)
    return bf16_round(x) if bf16 else x


def step(src_rows, islands, slots, master, mom, hp, first, bf16):
    """ga_diloco_outer_islands.  src_rows [S, n]: the values the source rows hold;
    islands: ascending row lists; slots[j][i]: the state row of member islands[j][i] or
    -1; master [K_state, n] fp32; mom [K_state, n] fp32 or None (momentum 0).  Returns
    (new master, new mom or None, {slot: the values x's row `slot` holds afterwards});
    rows of the state that no slot names come back unchanged."""
    src_rows = np.asarray(src_rows, f32)
    master = np.array(master, f32)
    mom = None if mom is None else np.array(mom, f32)
    x = {}
    for members, sl in zip(islands, slots):
        total = np.zeros(src_rows.shape[1], f32)
        for r in members:                                    # sum = 0.f + src_{r0} + ... (ascending)
            total = total + src_rows[r]
        avg = (total / f32(len(members))).astype(f32)        # avg = sum / float(s)
        for slot in sl:
            if slot < 0:                                     # hosted elsewhere: summed, not updated
                continue
            g = (master[slot] - avg).astype(f32)             # g = master - avg
            prev = None if (first or mom is None) else mom[slot]
            m, buf = outer_from_g(g, master[slot], prev, hp, first)  # ga_diloco_outer's update from g on
            master[slot] = m
            if buf is not None:
                mom[slot] = buf
            x[slot] = _store(m, bf16)                        # x_slot = T(master_slot)
    return master, mom, x


def draw(num_nodes, island_size):
    """FedAvg's draw (federated_averaging.py:27-51) from Python's `random` in its current
    state: the shuffled node ids cut into consecutive slices, each ascending.  One island
    of all nodes, and no draw, for island_size None or >= num_nodes."""
    ranks = list(range(num_nodes))
    if island_size is None or island_size >= num_nodes:
        return [ranks]
    random.shuffle(ranks)
    return [sorted(ranks[i:i + island_size]) for i in range(0, num_nodes, island_size)]


def run(X0, deltas, H, rounds, hp, bf16=False):
    """Replay over K rows that start as X0 [K, n], every node's master = X0[0]: at step t
    every row takes deltas[t] [K, n] (the inner step: x <- store(x + delta)); when
    t % H == 0 and t > 0 the islands rounds[t] (ascending node lists) take their step,
    every node on its own master and momentum, and continue from their masters.
    Returns one dict per step: rows [K, n], master [K, n], mom [K, n] (zeros until the
    first round)."""
    X = _store(np.array(X0, f32), bf16)
    K, n = X.shape
    master = np.tile(np.array(X[0], f32), (K, 1))
    has_mom = hp["momentum"] != 0
    mom = np.zeros((K, n), f32)
    first = True
    out = []
    for t, d in enumerate(deltas):
        X = _store((X + np.asarray(d, f32)).astype(f32), bf16)
        if t % H == 0 and t > 0:
            islands = rounds[t]
            master, nm, x = step(X, islands, islands, master, mom if has_mom else None, hp, first, bf16)
            if has_mom:
                mom = nm
            for slot, row in x.items():
                X[slot] = row
            first = False
        out.append(dict(rows=X.copy(), master=master.copy(), mom=mom.copy()))
    return out
