"""The reduce geometry's decisions (flearn_amd/csrc/fa_geometry.hpp) on the CPU: tests/geometry_probe.cpp
is compiled against the header alone and asked for the plan of every case of
tests/instantiation_cases.py at 256 CUs; the plan, formatted with that module's own name builders,
must be the case's target — the kernel the GPU test (tests/test_gpu_instantiations.py) then sees
launched.  Grids, the float16 geometry and the window split are pinned to literals recorded from the
host code before the decision was split from the launches."""
import subprocess
from pathlib import Path

import pytest

import instantiation_cases as ic

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "flearn_amd" / "csrc"
CUS = 256


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("geometry") / "geometry_probe"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(CSRC), "-I", str(REPO / "include"),
                    str(REPO / "tests" / "geometry_probe.cpp"), "-o", str(exe)], check=True)

    def ask(queries):
        out = subprocess.run([str(exe)], input="".join(q + "\n" for q in queries), capture_output=True, text=True,
                             check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [line.split() for line in out]

    return ask


def _plan(fields):
    family, rest = fields[0], [int(x) for x in fields[1:]]
    return dict(zip(("family", "V", "W", "D", "KG", "EPIB", "wide16", "grid"), [family] + rest))


def _name(case, p):
    if p["family"] == "rows":
        assert p["D"] == 64 // (p["V"] * p["W"])
        return ic.rows_name(case.mode, case.op, p["V"], p["W"])
    if p["family"] == "narrow":
        return ic.narrow_name(case.mode, case.op, p["D"])
    if p["family"] == "rowmajor":
        assert (p["V"], p["W"], p["D"]) == ((16, 4, 1) if p["wide16"] else (8, 8, 1))
        assert p["EPIB"] == (4 if p["wide16"] and case.op else 2)
        return ic.rowmajor_name(case.mode, case.op, bool(p["wide16"]), p["KG"])
    if p["family"] == "splitn":
        assert (p["W"], p["D"]) == (4, 8)
        return ic.splitn_name(case.mode, case.op)
    raise AssertionError(f"unexpected family {p['family']}")


def _f32_query(case):
    return f"f32 {case.mode} {case.op} {case.n} {ic.resolve_ncols(case, CUS)} {CUS} {case.grid} {int(case.reorder)}"


def test_every_stack_case_plans_its_target(probe):
    plans = [_plan(f) for f in probe([_f32_query(c) for c in ic.CASES])]
    wrong = [(c, _name(c, p)) for c, p in zip(ic.CASES, plans) if _name(c, p) != c.target]
    assert not wrong, wrong[:5]
    planned = {_name(c, p) for c, p in zip(ic.CASES, plans)}
    assert len(planned) == sum(ic.FAMILY_COUNTS[f] for f in ("rows", "rowmajor", "narrow", "splitn")) == 263


def test_grids_of_the_short_grid_and_fill_rule_cases(probe):
    """Grid 17 is taken as forced (a block runs out of pieces); a fused share just past 16 / 32 KiB
    (17 or 34 chunks per block on 192 blocks) moves to the 204 blocks that make it 16 / 32."""
    forced = [c for c in ic.CASES if c.grid == 17]
    assert len(forced) == 2
    for c, f in zip(forced, probe([_f32_query(c) for c in forced])):
        assert _plan(f)["grid"] == 17
    share = [c for c in ic.CASES if isinstance(c.ncols, tuple)]
    assert len(share) == 30 and {c.ncols for c in share} == {("share", 17), ("share", 34)}
    for c, f in zip(share, probe([_f32_query(c) for c in share])):
        assert _plan(f)["grid"] == 204, c


# (V, W, D, grid) by VMAX and the share: KiB of every row per block on 192 blocks (256 CUs)
_HALF = {
    16: {1: (1, 1, 16, 192), 2: (1, 4, 16, 192), 5: (2, 4, 8, 192), 9: (4, 4, 4, 192), 17: (8, 4, 2, 192),
         33: (16, 4, 1, 192), 65: (16, 4, 1, 195)},
    8: {1: (1, 1, 16, 192), 2: (1, 4, 16, 192), 5: (2, 4, 8, 192), 9: (4, 4, 4, 192), 17: (8, 4, 2, 192),
        33: (8, 4, 2, 192), 65: (8, 4, 2, 195)},
    4: {1: (1, 1, 16, 192), 2: (1, 4, 16, 192), 5: (2, 4, 8, 192), 9: (4, 4, 4, 192), 17: (4, 4, 4, 192),
        33: (4, 4, 4, 192), 65: (4, 4, 4, 195)},
}


def test_float16_geometry(probe):
    points = [(vmax, share) for vmax in _HALF for share in _HALF[vmax]]
    got = probe([f"f16 {vmax} {share * 192 * 512} {CUS}" for vmax, share in points])  # 512 halves per KiB
    for (vmax, share), f in zip(points, got):
        p = _plan(f)
        assert p["family"] == "rows_h16"
        assert (p["V"], p["W"], p["D"], p["grid"]) == _HALF[vmax][share], (vmax, share)


def test_every_float16_case_plans_its_target(probe):
    """The H16 cases of tests/instantiation_cases.py on their forced grid of 3: the share table of
    that module (1, 3, 7, 13, 27, 61, 130 chunks per block), VMAX by the mode."""
    cases = ic.H16_CASES
    got = [_plan(f) for f in probe([f"f16 {ic.H16_MODES[c.mode][2]} {c.n_cols} {CUS} {c.grid}" for c in cases])]
    for c, p in zip(cases, got):
        assert p["family"] == "rows_h16"
        assert ic.h16_name(c.mode, p["V"], p["D"], p["W"]) == c.target, c
        assert p["grid"] == min(c.grid, ic.h16_chunks(c.n_cols)) == (2 if c.share == 1 else 3), c
        assert -(-ic.h16_chunks(c.n_cols) // p["grid"]) == c.share
    assert len({c.target for c in cases}) == ic.FAMILY_COUNTS["rows_h16"] == 27


def test_float16_forced_grid_points(probe):
    """A forced grid changes the grid alone: V, W and D are those the same share has on the natural
    grid (_HALF above), and a forced 0 is the three-field query."""
    for vmax in _HALF:
        for share, (v, w, d, _) in _HALF[vmax].items():
            for forced in (1, 3, 7):
                p = _plan(probe([f"f16 {vmax} {share * forced * 512} {CUS} {forced}"])[0])
                assert (p["V"], p["W"], p["D"], p["grid"]) == (v, w, d, forced), (vmax, share, forced)
    pairs = [(f"f16 {vmax} {ncols} {cus}", f"f16 {vmax} {ncols} {cus} 0") for vmax in (16, 8, 4) for cus in (256, 304, 64)
             for ncols in (1, 513, 98_304, 6_400_003, 12_600_000)]
    for a, b in pairs:
        assert probe([a]) == probe([b]), a
    # a forced grid wider than the window: one block per chunk
    assert _plan(probe([f"f16 16 1025 {CUS} 160"])[0])["grid"] == 3


def test_float16_plan_restatement(probe):
    """ic.plan_f16, which the GPU tests name their expected launches with, is the header's rule:
    on the natural and on forced grids, for three CU counts."""
    points = [(vmax, ncols, cus, forced) for vmax in (16, 8, 4) for cus in (256, 304, 64) for forced in (0, 1, 2, 3, 5, 500)
              for ncols in (1, 7, 512, 513, 520, 1025, 8192, ic.h16_chunk_cols(27), ic.h16_chunk_cols(70), 98_305,
                            cus * 3 * 128 + 1, cus * 3 * 512 * 4 - 1029, cus * 3 * 512 * 16 - 1029, cus * 3 * 512 * 32 - 1029,
                            cus * 64 * 512 - 5, cus * 64 * 512 + 5)]
    got = probe([f"f16 {vmax} {ncols} {cus} {forced}" for vmax, ncols, cus, forced in points])
    for pt, f in zip(points, got):
        p = _plan(f)
        assert (p["V"], p["D"], p["W"], p["grid"]) == ic.plan_f16(*pt), pt


def test_window_split(probe):
    mi = 1 << 20
    want = {  # (op, columns): (windows, columns per window)
        (0, 8 * mi - 1): (1, 8 * mi - 1), (0, 8 * mi): (2, 4194560), (0, 16 * mi - 1): (2, 8388864),
        (0, 16 * mi): (1, 16 * mi),
        (1, 8 * mi - 1): (1, 8 * mi - 1), (1, 8 * mi): (1, 8 * mi), (1, 16 * mi - 1): (1, 16 * mi - 1),
        (1, 16 * mi): (3, 5592576),
    }
    got = probe([f"win {op} {ncols}" for op, ncols in want])
    for key, f in zip(want, got):
        assert (int(f[0]), int(f[1])) == want[key], key


def test_balanced_grid(probe):
    got = probe(["bal 0 2048", "bal 5 2048", "bal 2048 2048", "bal 5000 2048"])
    assert [int(f[0]) for f in got] == [1, 5, 2048, 2048]
