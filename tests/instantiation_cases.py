"""The case table of tests/test_gpu_instantiations.py and tests/test_gpu_half_instantiations.py: for
every reduce kernel instantiation the product library ships, one shape that reaches it; and the
names of the fold, finish, trim and Gram instantiations, which their own GPU tests compare with
fa_last_launch (tests/test_gpu_fold.py, test_gpu_trim.py, test_gpu_gram.py).

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
  reduce_kernel_rows_h16  <HP, DIV, V, D, W, NT>            fa_half.hpp; DIV an int (0 f64, 1 f32, 2 f16 result)
  fold_kernel_rows        <P, V, D, W, NT>                  fa_fold.hpp; D = 64 / (V * W), W = 4
  fold_kernel_elem        <P>
  fold_finish_kernel      <A, T, OP>                        accumulator and result element types
  trim_kernel_rows        <NP, W, NT>                       fa_trim.hpp
  trim_kernel_elem        <T>
  gram_kernel_tile        <NP, CEN, NT>                     fa_gram.hpp
"""
from collections import namedtuple

# fa_reduce_f32 modes (include/flearn_amd.h) -> accumulation policy P, epilogue precision T
MODES = {0: ("AccF32", "double"), 1: ("AccF32", "float"), 2: ("AccF32W64", "double")}
OPS = ("mean", "avgm", "adagrad", "yogi", "adam", "dyn")  # index = FA_OP_*
YOGI = 3

# Families whose launches fa_last_launch reports (the reduce families without their `reduce_kernel_`
# prefix): every instantiation has a target below
FAMILY_COUNTS = {"rows": 120, "rowmajor": 71, "narrow": 54, "rows_h16": 27, "splitn": 18, "segrows_rm": 18,
                 "balanced": 2, "fold_kernel_rows": 10, "fold_kernel_elem": 2, "fold_finish_kernel": 19,
                 "trim_kernel_rows": 6, "trim_kernel_elem": 2, "gram_kernel_tile": 8}
COVERED = tuple(FAMILY_COUNTS)
# Kernels that leave no launch record (the standalone update, the gathers, copies, pushes, fences,
# the fill and the Gram sum behind gram_kernel_tile): their instantiation counts only
UNRECORDED_COUNTS = {"apply_kernel": 10, "gather_rows_kernel": 3, "gather_rows_f64_kernel": 1, "copy_kernel": 1,
                     "push_kernel": 1, "cache_fence_kernel": 2, "fill_uniform_kernel": 1, "gram_finish_kernel": 1}

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

# ---------------------------------------------------------------------------------------------
# float16 stacks (fa_reduce_f16, reduce_kernel_rows_h16): tests/test_gpu_half_instantiations.py
# ---------------------------------------------------------------------------------------------

# fa_reduce_f16 modes (include/flearn_amd.h) -> accumulation policy HP, DIV, VMAX (fa_reduce.hip)
H16_MODES = {0: ("AccH16Pk", 0, 16), 1: ("AccH16Torch", 0, 16), 2: ("AccH16Pk", 2, 16), 3: ("AccH16W32", 1, 8),
             4: ("AccH16W64", 0, 4)}
H16_MODE_NAMES = ("numpy", "torch", "np16", "w32", "w64")  # index = FA_MODE_H16_*
H16_GRID = 3
# chunks (1 KiB = 512 halves of a row) per block on the forced grid -> (V, D, W); a policy whose
# VMAX is narrower runs its VMAX shape (VMAX, 16 / VMAX, 4) instead, in several rounds per block
# once the share passes 4 * VMAX.  Share 130: 389 chunks, for VMAX 16 three rounds of 44-chunk pieces
# (narrower than the 64-chunk slot).
H16_SHARES = {1: (1, 16, 1), 3: (1, 16, 4), 7: (2, 8, 4), 13: (4, 4, 4), 27: (8, 2, 4), 61: (16, 1, 4),
              130: (16, 1, 4)}
_H16_COL_BEGINS = (8, 24, 40, 72, 136, 520)  # non-zero multiples of 8

# n: clients; alone: also launch each output with the other two NULL
H16Case = namedtuple("H16Case", "target mode grid n n_cols col_begin share alone")


def h16_name(mode, v, d, w):
    hp, div, _ = H16_MODES[mode]
    return f"reduce_kernel_rows_h16<{hp},{div},{v},{d},{w},true>"


def h16_chunk_cols(chunks):
    """A window of exactly `chunks` 1-KiB chunks with an odd column count and a partial last oct."""
    return chunks * 512 - 509


def h16_chunks(n_cols):
    return -(-(-(-n_cols // 8)) // 64)


def h16_shape(mode, share):
    v, d, w = H16_SHARES[share]
    vmax = H16_MODES[mode][2]
    return (v, d, w) if v <= vmax else (vmax, 16 // vmax, 4)


def h16_rounds(target, grid, n_cols):
    """k of reduce_kernel_rows_h16 (fa_half.hpp): the rounds in which `grid` blocks of the launched
    (V, W) sweep the window."""
    v, _, w = (int(x) for x in target[target.index("<") + 1 : -1].split(",")[2:5])
    return -(-h16_chunks(n_cols) // (grid * w * v))


def plan_f16(vmax, n_cols, cus, forced=0):
    """plan_f16_window (fa_geometry.hpp) restated: (V, D, W, grid).  tests/test_geometry_plan.py holds
    it equal to the header; the GPU tests use it for the name a shape reaches on the device's CUs."""
    chunks = h16_chunks(n_cols)
    grid = forced if forced > 0 else int(cus * 0.75 + 0.5)
    if forced <= 0 and grid * 64 < chunks <= cus * 64:
        grid = -(-chunks // 64)
    grid = min(max(grid, 1), chunks)
    share = -(-chunks // grid)
    w = 1 if share <= 1 else 4
    v = 1
    while v < vmax and share > v * w:
        v *= 2
    return v, (1 if v * w >= 64 else min(16, 64 // (v * w))), w, grid


def h16_plan_name(mode, n_cols, cus, forced=0):
    """(name, grid) of the launch fa_reduce_f16 makes for the window."""
    v, d, w, grid = plan_f16(H16_MODES[mode][2], n_cols, cus, forced)
    return h16_name(mode, v, d, w), grid


def _h16_cases():
    """Per (mode, share) two cases: n = 2D + 1 (ramp, one steady round, the first drain), and one
    of n = 1, D, D + 1 in rotation (no pipeline, the ramp alone, both drain loops)."""
    out = []
    for mode in H16_MODES:
        for share in H16_SHARES:
            v, d, w = h16_shape(mode, share)
            chunks = H16_GRID * share - 1
            extra = (1, d, d + 1)[len(out) // 2 % 3]
            for n in (2 * d + 1, extra):
                out.append(H16Case(h16_name(mode, v, d, w), mode, H16_GRID, n, h16_chunk_cols(chunks),
                                   _H16_COL_BEGINS[len(out) % len(_H16_COL_BEGINS)], share,
                                   share == 130 and n == 2 * d + 1))
    return out


H16_CASES = _h16_cases()

# ---------------------------------------------------------------------------------------------
# streamed rounds, trimmed sums, the Gram matrix: names only (their GPU tests hold the shapes)
# ---------------------------------------------------------------------------------------------

FOLD_ROWS_POLICY = {0: "AccF32", 1: "AccF32W64"}  # FA_ACC_F32, FA_ACC_F32_W64
FOLD_ELEM = {2: "fold_kernel_elem<AccF64>", 3: "fold_kernel_elem<AccI64>"}  # FA_ACC_F64, FA_ACC_I64
FOLD_V = (1, 2, 4, 8, 16)


def fold_rows_name(acc_kind, v):
    return f"fold_kernel_rows<{FOLD_ROWS_POLICY[acc_kind]},{v},{64 // (4 * v)},4,true>"


def fold_finish_name(acc_kind, mode, op):
    """fa_fold_finish: the accumulator's element type by the kind, the result's by the mode."""
    a = {0: "float", 1: "double", 2: "double", 3: "long"}[acc_kind]
    t = "float" if (acc_kind == 0 and mode == 1) else "double"
    return f"fold_finish_kernel<{a},{t},{op}>"


FOLD_TARGETS = (frozenset(fold_rows_name(k, v) for k in FOLD_ROWS_POLICY for v in FOLD_V) | frozenset(FOLD_ELEM.values())
                | frozenset(fold_finish_name(k, m, op) for k, m in ((0, 0), (0, 1), (1, 2)) for op in range(6))
                | frozenset(fold_finish_name(k, 0, 0) for k in (2, 3)))

TRIM_NP = (4, 8, 16, 32, 64, 128)
TRIM_ELEM = {2: "trim_kernel_elem<double>", 3: "trim_kernel_elem<long>"}  # FA_ACC_F64, FA_ACC_I64


def trim_rows_name(np_):
    assert np_ in TRIM_NP
    return f"trim_kernel_rows<{np_},4,true>"


TRIM_TARGETS = frozenset(map(trim_rows_name, TRIM_NP)) | frozenset(TRIM_ELEM.values())

GRAM_NP = (32, 64, 96, 128)


def gram_name(np_, centred):
    assert np_ in GRAM_NP
    return f"gram_kernel_tile<{np_},{_b(centred)},true>"


GRAM_TARGETS = frozenset(gram_name(np_, c) for np_ in GRAM_NP for c in (False, True))

TARGETS = (frozenset(c.target for c in CASES) | frozenset(SEGROWS_TARGETS.values()) | frozenset(BALANCED.values())
           | frozenset(c.target for c in H16_CASES) | FOLD_TARGETS | TRIM_TARGETS | GRAM_TARGETS)
