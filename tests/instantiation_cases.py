"""The case table of tests/test_gpu_instantiations.py: for every reduce kernel instantiation the
product library ships (float16 family aside: tests/test_gpu_half.py), one shape that reaches it.

A plain module (no torch, no GPU): tests/test_kernel_inventory.py compares TARGETS with the
instantiations in the built library, in both directions, so a kernel added to the dispatch
without a case here — or a case naming a kernel that is no longer shipped — fails on a CPU box.
The GPU test then asserts, per case, that the library's launch record names exactly `target`;
the names below are claims it checks, not a second implementation of the geometry.

Names are the demangled kernel symbols without `fa::`, whitespace and the argument list (what
fa_last_launch reports).  Template arguments, as in flearn_amd/csrc/fa_device.hpp:
  reduce_kernel_rows      <P, T, OP, V, D, W, NT>           D = 64 / (V * W)
  reduce_kernel_narrow    <P, T, OP, D, W, NT>
  reduce_kernel_rowmajor  <P, T, OP, V, D, W, KG, NT, EPIB, TR, XL>
  reduce_kernel_splitn    <P, T, OP, W, D, NT>
  reduce_kernel_segrows_rm<P, T, OP, V, W, KG, DN, NT, TR, XLS>
  reduce_kernel_balanced  <P, T, OP, V, U, NT>
"""
from collections import namedtuple

# fa_reduce_f32 modes (include/flearn_amd.h) -> accumulation policy P, epilogue precision T
MODES = {0: ("AccF32", "double"), 1: ("AccF32", "float"), 2: ("AccF32W64", "double")}
OPS = ("mean", "avgm", "adagrad", "yogi", "adam", "dyn")  # index = FA_OP_*
YOGI = 3

FAMILY_COUNTS = {"rows": 120, "rowmajor": 71, "narrow": 54, "rows_h16": 27, "splitn": 18, "segrows_rm": 18,
                 "balanced": 2}
COVERED = ("rows", "rowmajor", "narrow", "splitn", "segrows_rm", "balanced")

NONDEFAULT = dict(beta=0.7, eta=0.03, tau=1e-3, beta2=0.9)

# grid: fa_set_reduce_grid (0 = the library's geometry).  ncols: columns, or ("share", s): the
# window of s * round(0.75 * CUs) - 5 one-KiB chunks, i.e. s chunks per block on the natural grid.
# reorder: fa_reduce_f32_splitn.  hyper: NONDEFAULT instead of the reference's defaults.
Case = namedtuple("Case", "target grid mode op n ncols col_begin reorder hyper")


def chunk_cols(chunks):
    """A window of exactly `chunks` 1-KiB chunks whose last quad is ragged (ncols % 4 == 3)."""
    return chunks * 256 - 253


def resolve_ncols(case, cus):
    if isinstance(case.ncols, tuple):
        return chunk_cols(case.ncols[1] * int(cus * 0.75 + 0.5) - 5)
    return case.ncols


def _b(x):
    return "true" if x else "false"


def rows_name(mode, op, v, w):
    p, t = MODES[mode]
    return f"reduce_kernel_rows<{p},{t},{op},{v},{64 // (v * w)},{w},true>"


def narrow_name(mode, op, d):
    p, t = MODES[mode]
    return f"reduce_kernel_narrow<{p},{t},{op},{d},1,true>"


def rowmajor_name(mode, op, wide16, kg):
    p, t = MODES[mode]
    xl = _b(t == "double" and op != 0 and kg <= 3)
    if wide16:
        return f"reduce_kernel_rowmajor<{p},{t},{op},16,1,4,{kg},true,{2 if op == 0 else 4},false,{xl}>"
    return f"reduce_kernel_rowmajor<{p},{t},{op},8,1,8,{kg},true,2,false,{xl}>"


def splitn_name(mode, op):
    p, t = MODES[mode]
    return f"reduce_kernel_splitn<{p},{t},{op},4,8,true>"


def segrows_name(mode, op):
    p, t = MODES[mode]
    kg, xls = 1 if mode == 2 else 2, _b(t == "double" and op != 0)
    return f"reduce_kernel_segrows_rm<{p},{t},{op},8,8,{kg},16,true,false,{xls}>"


BALANCED = {"f64": "reduce_kernel_balanced<AccF64,double,0,4,1,true>",
            "i64": "reduce_kernel_balanced<AccI64,double,0,4,1,true>"}

_COL_BEGINS = (4, 12, 20, 28, 44, 260)  # 4 x an odd number


def _cases():
    out = []
    seen_hyper = set()

    def add(family, target, grid, mode, op, n, ncols, reorder=False):
        hyper = op != 0 and (family, op) not in seen_hyper  # one target per (family, op)
        if hyper:
            seen_hyper.add((family, op))
        out.append(Case(target, grid, mode, op, n, ncols, _COL_BEGINS[len(out) % len(_COL_BEGINS)], reorder, hyper))

    # ---- row-major groups (fp32 sums only), forced grid 3: k = ceil(chunks / (64 * 3)) pieces per
    # block.  k = 2, 3, 4: groups of KG = k on 8 waves x 8 KiB; k = 6, 8, 10: KG = 3, 4, 2 on 4 waves
    # x 16 KiB; k = 5 (KG 3) and k = 7 (KG 4): the last group has a missing slot.  Yogi's f64
    # epilogue stays on 8 waves at KG = 4.  n = 5 = 2 * D + 3 (D = 1).  The window is the narrowest
    # of its k (7 chunks past k - 1 full rounds), so the last piece is short and ragged.
    k_to = {2: (False, 2), 3: (False, 3), 4: (False, 4), 5: (False, 3), 6: (True, 3), 7: (True, 4), 8: (True, 4),
            10: (True, 2)}
    for mode in (0, 1):
        for op in range(6):
            for k, (wide16, kg) in k_to.items():
                if wide16 and kg == 4 and op == YOGI and mode == 0:
                    wide16 = False
                add("rowmajor", rowmajor_name(mode, op, wide16, kg), 3, mode, op, 5, chunk_cols(64 * 3 * (k - 1) + 7))
    # a grid on which a block runs out of pieces: 17 blocks, k = 2, 1089 chunks in 33 pieces of 33
    add("rowmajor", rowmajor_name(0, 0, False, 2), 17, 0, 0, 5, chunk_cols(1089))
    add("rowmajor", rowmajor_name(1, 1, False, 2), 17, 1, 1, 5, chunk_cols(1089))
    # n = 1 and n = 2
    add("rowmajor", rowmajor_name(0, 1, False, 3), 3, 0, 1, 1, chunk_cols(64 * 3 * 2 + 7))
    add("rowmajor", rowmajor_name(1, 5, True, 3), 3, 1, 5, 2, chunk_cols(64 * 3 * 5 + 7))
    add("rowmajor", rowmajor_name(0, 0, True, 2), 3, 0, 0, 1, chunk_cols(64 * 3 * 9 + 7))

    # ---- one piece per block (reduce_kernel_rows), forced grid: `share` chunks per block picks
    # (V, W); n = 2 * D + 3, D = 64 / (V * W).  Grid 1 for DIV64; grid 2 (two blocks, the second
    # one's piece short) for DIV32 and W64.
    mean_vw = {3: (1, 4), 7: (2, 4), 13: (4, 4), 27: (8, 4), 61: (16, 4)}
    fused_vw = {3: (1, 4), 7: (2, 4), 13: (2, 8), 27: (4, 8), 61: (8, 8)}
    for mode in (0, 1, 2):
        g = 1 if mode == 0 else 2
        for op in range(6):
            for share, (v, w) in (mean_vw if op == 0 else fused_vw).items():
                chunks = share if g == 1 else 2 * share - 1
                add("rows", rows_name(mode, op, v, w), g, mode, op, 2 * (64 // (v * w)) + 3, chunk_cols(chunks))
            if op:
                # the fused fill rule, natural grid only: a share just past 16 / 32 KiB takes the grid
                # that makes it a whole 16 / 32 KiB piece on 4 waves
                add("rows", rows_name(mode, op, 4, 4), 0, mode, op, 2, ("share", 17))
                add("rows", rows_name(mode, op, 8, 4), 0, mode, op, 2, ("share", 34))
    add("rows", rows_name(0, 0, 1, 4), 1, 0, 0, 1, chunk_cols(3))
    add("rows", rows_name(1, 2, 2, 8), 2, 1, 2, 2, chunk_cols(25))
    add("rows", rows_name(2, 5, 8, 8), 2, 2, 5, 1, chunk_cols(121))

    # ---- narrow windows (at most two chunks per block): D by the client count
    for mode in (0, 1, 2):
        for op in range(6):
            for d, n in ((16, 35), (32, 350), (40, 703)):
                add("narrow", narrow_name(mode, op, d), 0, mode, op, n, 517)
    add("narrow", narrow_name(0, 0, 16), 0, 0, 0, 349, 301)
    add("narrow", narrow_name(1, 1, 32), 0, 1, 1, 699, 301)
    add("narrow", narrow_name(2, 4, 16), 0, 2, 4, 1, 517)
    add("narrow", narrow_name(0, 3, 16), 0, 0, 3, 2, 259)
    add("narrow", narrow_name(0, 0, 16), 1, 0, 0, 35, chunk_cols(2))  # forced grid 1, two chunks a block

    # ---- split-N (8 <= n <= 256, fewer chunks than CUs): 4 splits, each a pipeline 8 rows deep;
    # n = 77 gives every split 19 = 2 * 8 + 3 rows or one more
    for mode in (0, 1, 2):
        for op in range(6):
            add("splitn", splitn_name(mode, op), 0, mode, op, 77, (517, 259, 131)[op % 3], reorder=True)
    add("splitn", splitn_name(0, 0), 0, 0, 0, 8, 517, reorder=True)
    add("splitn", splitn_name(2, 1), 0, 2, 1, 9, 259, reorder=True)
    add("splitn", splitn_name(1, 2), 0, 1, 2, 256, 131, reorder=True)
    return out


CASES = _cases()

# the row-pointer kernel: (mode by weight kind) x (strategy), tests/test_gpu_instantiations.py
SEGROWS_WEIGHTS = {"pyfloat": 0, "np32": 1, "np64": 2}
SEGROWS_TARGETS = {(wk, op): segrows_name(mode, op) for wk, mode in SEGROWS_WEIGHTS.items() for op in range(6)}

TARGETS = frozenset(c.target for c in CASES) | frozenset(SEGROWS_TARGETS.values()) | frozenset(BALANCED.values())
