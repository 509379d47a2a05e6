"""The streamed clipped round's kernel restated for its tests: the table of shipped fa::clipfold
instantiations as fa_last_launch spells them, the shapes that reach each (clip_ref.COVER: the plan
is plan_fold_window's, as for clip_sum_kernel), and the chained clipped sum in numpy — clip_ref's
clipped_upload row by row, the fp32 sum continuing across the chunks.  No torch, no flearn_amd."""
import numpy as np

import clip_ref as cr

FAMILY = "clip_fold_kernel"
VS = cr.VS
COVER = cr.COVER  # V -> (columns, forced grid)
TARGETS = {cr.instance(FAMILY, v) for v in VS}


def chunks_of(n, splits):
    """[(begin, end)] of the chunks rows [0, n) are cut into at the row indices `splits`."""
    cuts = [0, *sorted(splits), n]
    assert all(a < b for a, b in zip(cuts, cuts[1:])), "splits must be strictly inside (0, n) and distinct"
    return list(zip(cuts, cuts[1:]))


def fold_chunk(acc, rows, g, scale):
    """fp32 [cols]: one chunk.  acc None: the chunk opens the round (row 0's clipped upload is the
    sum); else every row's clipped upload is added to acc, in list order."""
    start = 0
    if acc is None:
        acc, start = cr.clipped_upload(rows[0], g, scale[0]), 1
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(start, len(rows)):
            acc = (acc + cr.clipped_upload(rows[i], g, scale[i])).astype(np.float32)
    return acc


def fold_chain(stack, g, scale, splits):
    """fp32 [cols]: the clipped sum of the rows of `stack`, made chunk by chunk."""
    acc = None
    for a, b in chunks_of(len(stack), splits):
        acc = fold_chunk(acc, stack[a:b], g, scale[a:b])
    return acc
