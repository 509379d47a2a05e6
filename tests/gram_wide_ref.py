"""plan_gram_wide (flearn_amd/csrc/fa_gramwide_geometry.hpp) restated in Python; tests/test_gram_wide_host.py
pins it to the header through tests/gram_wide_geometry_probe.cpp, and the GPU tests take `chain` and
`slices` of a launch from it.  The numpy reference and gamma are tests/gram_ref.py's."""
from typing import NamedTuple

import numpy as np

import gram_ref as gr

MAX_CLIENTS, PANEL, KC, LC = 1024, 128, 64, gr.LC
ROUNDS, UNIT_CAP, SLOT = 4, 2048, 128 * 128 * 4


class GramWidePlan(NamedTuple):
    tiles: int
    panels: int
    pairs: int
    kc: int
    lc: int
    chunks: int
    slices: int
    share: int
    chain: int
    workspace_bytes: int


def plan(n_clients, n_cols, cus, forced=0):
    if n_clients < 1 or n_clients > MAX_CLIENTS:
        return GramWidePlan(0, 0, 0, KC, LC, 0, 0, 0, 0, 0)
    panels = -(-n_clients // PANEL)
    pairs = panels * (panels + 1) // 2
    chunks = -(-max(n_cols, 1) // KC)
    slices = max(1, min(forced if forced > 0 else ROUNDS * cus // pairs, UNIT_CAP // pairs, chunks))
    share = -(-chunks // slices) * KC
    return GramWidePlan(-(-n_clients // 32), panels, pairs, KC, LC, chunks, slices, share, LC + -(-share // LC),
                        slices * pairs * SLOT)


def launch_plan(n_clients, n_cols, cus, forced=0):
    """The plan fa_gram_f32_wide launches with on a device of `cus` CUs under fa_set_reduce_grid(forced)."""
    return plan(n_clients, n_cols, min(cus, UNIT_CAP // ROUNDS), min(forced, UNIT_CAP))


def workspace_bytes(n_clients, n_cols):
    """fa_gram_wide_workspace past 128 clients."""
    panels = -(-n_clients // PANEL)
    return min(-(-min(n_cols, UNIT_CAP * KC) // KC) * (panels * (panels + 1) // 2), UNIT_CAP) * SLOT


def bound(x, c, p):
    """|G - G_ref| <= gamma(chain) * S + slices * 2^-52 * S, S = |y64| @ |y64|.T: gram_ref.bound with
    the slices of an entry in place of the blocks."""
    y = np.abs(gr.centred(x, c).astype(np.float64))
    s = y @ y.T
    return gr.gamma(p.chain) * s + p.slices * 2.0 ** -52 * s
