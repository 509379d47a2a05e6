"""Host-only: the Gaussian noise of a DP-FedAvg round.  tests/noise_ref.py's
Philox against known answers and its normals against the statistical conditions the GPU values must
pass too; plan_gauss_add (tests/noise_geometry_probe.cpp against flearn_amd/csrc/fa_geometry.hpp
alone, and its Python restatement); the ABI 21 surface and every refusal of fa_gauss_add_f32 (decided
before any HIP call); and the refusals of clip.check_noise, Aggregator.ensemble_clipped and the
NormClip strategy, raised before the engine touches a device.  No GPU."""
import inspect
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import flearn_amd
import flearn_amd.aggregator
import noise_ref as nr
from flearn_amd import _native as na
from flearn_amd import clip
from test_clip_host import bare_engine, header_define, nothing_launched, uploads

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "flearn_amd" / "csrc"
HEADER = REPO / "include" / "flearn_amd.h"
CUS = (256, 304, 64)


# ---------------------------------------------------------------------------------------------
# the restatement itself
# ---------------------------------------------------------------------------------------------

KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def test_philox_known_answers():
    for counter, key, want in KNOWN:
        assert " ".join(f"{int(w):08x}" for w in nr.philox4x32(counter, key)) == want
    # arrays of counters give each counter's own words, and the counter / key layout is section 15's
    c = np.array([k[0] for k in KNOWN], dtype=np.uint64).T
    assert [f"{int(w):08x}" for w in np.asarray(nr.philox4x32(tuple(c), (0, 0)))[:, 0]] == KNOWN[0][2].split()
    seed, seq, q = 0x299F31D0A4093822, 0x0370734413198A2E, 0x85A308D3243F6A88
    assert " ".join(f"{int(w):08x}" for w in nr.words(seed, seq, [q])[0]) == KNOWN[2][2]


def test_uniforms_are_exact_and_open():
    w = np.array([0, 511, 512, 0xFFFFFFFF, 0xFFFFFE00, 95, 481], dtype=np.uint64)
    u = nr.uniform(w)
    assert u.min() == 2.0 ** -24 and u.max() == 1 - 2.0 ** -24 and u[2] == 1.5 * 2.0 ** -23
    assert (u.astype(np.float32).astype(np.float64) == u).all()  # exact in fp32
    assert math.sqrt(-2 * math.log(u.min())) == pytest.approx(nr.Z_MAX, abs=1e-14) and abs(nr.Z_MAX - 5.768) < 1e-3
    assert 0 < nr.Z_ERROR <= 1e-5


def conditions(z, z_other):
    """The three statistical conditions of section 15 on n standard normals (and a second draw)."""
    n = z.size
    lim = 5 / math.sqrt(n)
    mean, var = float(z.mean()), float(z.var())
    lag1 = float(np.corrcoef(z[:-1], z[1:])[0, 1])
    cross = float(np.corrcoef(z, z_other)[0, 1])
    print(f"n {n}: mean {mean:.3g} (<= {lim:.3g}), var {var:.6g} (|var - 1| <= {5 * math.sqrt(2 / n):.3g}), "
          f"max |z| {np.abs(z).max():.6g}, lag-1 {lag1:.3g}, sequence 1 against 2 {cross:.3g}")
    assert abs(mean) <= lim and abs(var - 1) <= 5 * math.sqrt(2 / n)
    assert np.abs(z).max() <= 5.7682
    assert abs(lag1) <= lim and abs(cross) <= lim


def test_reference_normals_pass_the_statistical_conditions():
    s = nr.SAMPLE
    assert (s["seed"], s["sequence"], s["n"]) == (0x0123456789ABCDEF, 1, 1 << 20)
    conditions(nr.normals(s["seed"], 1, 0, s["n"]), nr.normals(s["seed"], 2, 0, s["n"]))


def test_a_columns_normal_is_its_own():
    s = nr.SAMPLE
    z = nr.normals(s["seed"], 1, 0, 64)
    for c0, n in ((0, 1), (1, 6), (3, 2), (4, 8), (61, 3)):
        assert nr.normals(s["seed"], 1, c0, n).tobytes() == z[c0 : c0 + n].tobytes()
    hi = nr.normals(s["seed"], 1, 2 ** 34, 8)
    assert np.isfinite(hi).all() and not np.array_equal(hi, nr.normals(s["seed"], 1, 0, 8))  # the high counter word counts
    assert not np.array_equal(z[:8], nr.normals(s["seed"] + 1, 1, 0, 8))
    # the edge uniforms section 15 names
    w = nr.words(s["seed"], 1, [3939685, 18031565])
    assert int(w[0, 2]) == 481 and int(w[1, 0]) == 95
    edge = nr.normals(s["seed"], 1, 15758742, 2)
    assert math.hypot(*edge) == pytest.approx(nr.Z_MAX, abs=1e-12)


def test_add_rounds_twice():
    acc = np.array([1.0, -0.0, 3e-8, 1e8], np.float32)
    z = np.array([0.3, 0.0, 1.7, -2.5], np.float32)
    got = nr.add(acc, 0.1, z)
    assert got.dtype == np.float32
    want = [np.float32(np.float32(a) + np.float32(np.float32(0.1) * zz)) for a, zz in zip(acc, z)]
    assert got.tobytes() == np.array(want, np.float32).tobytes()


# ---------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("noise_geometry") / "noise_geometry_probe"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(CSRC), "-I", str(REPO / "include"),
                    str(REPO / "tests" / "noise_geometry_probe.cpp"), "-o", str(exe)], check=True)

    def ask(queries):
        out = subprocess.run([str(exe)], input="".join(q + "\n" for q in queries), capture_output=True, text=True,
                             check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [[int(x) for x in f.split()] for f in out]

    return ask


WIDTHS = sorted({0, 1, 3, 4, 5, 255, 1023, 1024, 1025, 4093, 70001, 1 << 20, 25_610_152, 2 ** 40 + 1, 2 ** 63 - 1})
FORCED = (0, 1, 3, 100000)


@pytest.mark.parametrize("cus", CUS)
def test_plan_gauss_add(cus, probe):
    qs = [(w, f) for w in WIDTHS for f in FORCED]
    plans = probe([f"plan {w} {cus} {f}" for w, f in qs])
    small = [(w, f) for w, f in qs if w <= 70001]
    covers = dict(zip(small, probe([f"cover {w} {cus} {f}" for w, f in small])))
    for (w, f), got in zip(qs, plans):
        quads, blocks, grid, steps = got
        assert tuple(got) == tuple(nr.plan(w, cus, f)), (w, f)  # the restatement the GPU tests use
        assert quads == -(-w // 4) and blocks == max(1, -(-quads // 256))
        assert 1 <= grid <= blocks and grid <= (f if f else cus * 8) and steps == -(-blocks // grid)
        if blocks <= (f if f else cus * 8):
            assert grid == blocks and steps == 1
        if (w, f) in covers:  # every column of the window is written once, none outside it
            bad, outside, busiest = covers[(w, f)]
            assert bad == 0 and outside == 0 and busiest == (steps if w else 0)
    assert probe([f"plan -5 {cus} 0"]) == [[0, 1, 1, 1]]


# ---------------------------------------------------------------------------------------------
# ABI 21
# ---------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def L():
    return na.load()


def test_abi_surface(L):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fa_[a-z0-9_]+)\s*\(", text))) == sorted(na.EXPORTS)
    assert re.search(r"\bint\s+fa_gauss_add_f32\s*\(\s*float\s*\*\s*acc,\s*int64_t\s+col_begin,\s*int64_t\s+n_cols,\s*float\s+sigma,"
                     r"\s*uint64_t\s+seed,\s*uint64_t\s+sequence,\s*void\s*\*\s*stream\s*\)", text)
    assert L.fa_abi_version() == header_define("FA_ABI_VERSION") == na.ABI_VERSION >= 21
    out = subprocess.run(["nm", "-D", "--defined-only", str(na.LIB_PATH)], capture_output=True, text=True).stdout
    assert "fa_gauss_add_f32" in na.EXPORTS and hasattr(L, "fa_gauss_add_f32")
    assert re.search(r"\bT\s+fa_gauss_add_f32$", out, flags=re.M)
    whole = HEADER.read_text()
    assert "fa_gauss_add_f32" in whole[whole.index("call launched") - 300 : whole.index("call launched")]  # fa_last_launch's list
    from flearn_amd import _build

    assert CSRC / "fa_noise.hip" in _build.SOURCES and (CSRC / "fa_noise.hpp").exists()


FAKE = 0x100000  # never dereferenced: validation rejects the call first, or nothing is launched


def test_gauss_add_refusals_need_no_gpu(L):
    arg, align = header_define("FA_ERR_ARG"), header_define("FA_ERR_ALIGN")

    def call(acc=FAKE, col=0, ncols=64, sigma=1.0, seed=1, seq=2):
        rc = L.fa_gauss_add_f32(acc, col, ncols, sigma, seed, seq, None)
        nothing_launched(L)
        return rc

    assert call(acc=None) == arg and b"null" in L.fa_last_error()
    assert call(acc=None, ncols=1) == arg
    assert call(ncols=-1) == arg and b"window" in L.fa_last_error()
    assert call(col=-4) == arg and call(col=-1) == arg and call(ncols=-(2 ** 63)) == arg
    for bad in (-1.0, -1e-30, math.nan, math.inf, -math.inf):
        assert call(sigma=bad) == arg and b"sigma" in L.fa_last_error(), bad
    assert call(acc=FAKE + 4) == align and call(acc=FAKE + 8) == align and b"aligned" in L.fa_last_error()
    assert call(col=2) == align and call(col=1) == align and call(col=2 ** 40 + 2) == align
    assert call(acc=FAKE + 4, ncols=-1) == arg  # an argument error wins over an alignment error, as for fa_fold
    assert call(acc=FAKE + 4, sigma=-1.0) == arg
    # no-ops launch nothing: an empty window (a NULL accumulator allowed) and sigma = 0 (-0.0 included)
    assert call(ncols=0) == 0 and call(acc=None, ncols=0) == 0 and call(sigma=0.0) == 0 and call(sigma=-0.0) == 0
    assert call(ncols=0, col=2 ** 62) == 0 and call(sigma=0.0, seed=2 ** 64 - 1, seq=2 ** 64 - 1) == 0
    assert call(acc=FAKE + 4, ncols=0) == align  # but a no-op's arguments are still checked


def test_ops_entry_signature():
    from flearn_amd import ops

    sig = inspect.signature(ops.gauss_add)
    assert list(sig.parameters) == ["acc", "sigma", "seed", "sequence", "col_begin", "n_cols"]
    assert [p.kind for p in sig.parameters.values()][4:] == [inspect.Parameter.KEYWORD_ONLY] * 2
    assert sig.parameters["col_begin"].default == 0 and sig.parameters["n_cols"].default is None
    with pytest.raises(ValueError, match="device tensor"):
        ops.gauss_add(np.zeros(4, np.float32), 1.0, 1, 1)


# ---------------------------------------------------------------------------------------------
# what a noised round refuses: before a device is touched
# ---------------------------------------------------------------------------------------------


def test_check_noise():
    assert clip.check_noise(None, None, 0, 1.0, None, True) is None
    assert clip.check_noise(0, None, 0, None, 0.5, False) is None and clip.check_noise(0.0, 5, 0, math.inf, None, True) is None
    assert clip.check_noise(1.5, 7, 3, 2.0, None, True) == (1.5, 3.0, 7, 3)
    m, sigma, seed, seq = clip.check_noise(np.float32(0.1), np.int64(2 ** 40), np.uint64(2 ** 64 - 1), 0.3, None, True)
    assert sigma == float(np.float32(float(np.float32(0.1)) * 0.3)) and type(sigma) is float
    assert (seed, seq) == (2 ** 40, 2 ** 64 - 1) and type(seed) is int and type(seq) is int
    for bad in (-1.0, -1e-300, math.nan, math.inf, -math.inf, True, "1", [1.0]):
        with pytest.raises(ValueError, match="noise_multiplier"):
            clip.check_noise(bad, 1, 0, 1.0, None, True)
    with pytest.raises(ValueError, match="quantile"):
        clip.check_noise(1.0, 1, 0, None, 0.5, True)
    with pytest.raises(ValueError, match="finite tau"):
        clip.check_noise(1.0, 1, 0, math.inf, None, True)
    with pytest.raises(ValueError, match="centre"):
        clip.check_noise(1.0, 1, 0, 1.0, None, False)
    for bad in (None, -1, 2 ** 64, 1.0, True, "7"):
        with pytest.raises(ValueError, match="seed"):
            clip.check_noise(1.0, bad, 0, 1.0, None, True)
        with pytest.raises(ValueError, match="sequence"):
            clip.check_noise(1.0, 1, bad, 1.0, None, True)
    for mult, tau in ((1e30, 1e30), (1e-30, 1e-30)):  # sigma leaves fp32's range
        with pytest.raises(ValueError, match="sigma"):
            clip.check_noise(mult, 1, 0, tau, None, True)


def test_engine_refusals_touch_no_device():
    ups = uploads(7)
    good = {k: np.zeros_like(v) for k, v in ups[0].items()}
    eng = bare_engine
    with pytest.raises(ValueError, match="quantile"):
        eng().ensemble_clipped(ups, None, 0.5, center=good, noise_multiplier=1.0, seed=1)
    with pytest.raises(ValueError, match="finite tau"):
        eng().ensemble_clipped(ups, math.inf, None, center=good, noise_multiplier=1.0, seed=1)
    with pytest.raises(ValueError, match="centre"):
        eng().ensemble_clipped(ups, 1.0, None, center=None, noise_multiplier=1.0, seed=1)
    for bad in (-0.5, math.nan, math.inf, "1", True):
        with pytest.raises(ValueError, match="noise_multiplier"):
            eng().ensemble_clipped(ups, 1.0, None, center=good, noise_multiplier=bad, seed=1)
    with pytest.raises(ValueError, match="seed"):
        eng().ensemble_clipped(ups, 1.0, None, center=good, noise_multiplier=1.0)
    with pytest.raises(ValueError, match="sequence"):
        eng().ensemble_clipped(ups, 1.0, None, center=good, noise_multiplier=1.0, seed=1, sequence=-1)
    # the round's other refusals still come first or apply as ever
    with pytest.raises(ValueError, match="chunk_clients"):
        eng(chunk_clients=4).ensemble_clipped(ups, 1.0, None, center=good, noise_multiplier=1.0, seed=1)
    with pytest.raises(TypeError, match="float16"):
        eng().ensemble_clipped(uploads(7, np.float16), 1.0, None, center=good, noise_multiplier=1.0, seed=1)
    for kw in ({"noise_multiplier": 1.0, "seed": 1}, {"noise_multiplier": 0}, {"noise_multiplier": None}):
        with pytest.raises(AssertionError, match="touched its packer"):  # a good round gets as far as the pack
            eng().ensemble_clipped(ups, 1.0, None, center=good, **kw)
    params = inspect.signature(flearn_amd.aggregator.Aggregator.ensemble_clipped).parameters
    assert list(params)[-3:] == ["noise_multiplier", "seed", "sequence"]
    assert [params[k].default for k in list(params)[-3:]] == [None, None, 0]


def test_strategy_surface_and_refusals():
    from flearn_amd.strategy import NormClip

    params = inspect.signature(NormClip.__init__).parameters
    new = ["noise_multiplier", "seed", "sequence"]
    assert list(params)[-3:] == new and all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in new)
    assert [params[k].default for k in new] == [None, None, 0]
    assert list(params)[1:5] == ["tau", "quantile", "server_opt", "center"]  # the existing ones keep their places
    s = NormClip(tau=2.0)
    assert s.noise_multiplier is None and s.sequence == 0 and not s._noised
    a, b = NormClip(tau=2.0, noise_multiplier=1.0), NormClip(tau=2.0, noise_multiplier=1.0)
    assert a._noised and 0 <= a.seed < 2 ** 64 and isinstance(a.seed, int) and a.seed != b.seed  # drawn at construction
    s = NormClip(tau=2.0, noise_multiplier=0.5, seed=11, sequence=4)
    assert (s.noise_multiplier, s.seed, s.sequence) == (0.5, 11, 4)
    assert not NormClip(tau=2.0, noise_multiplier=0, seed=11)._noised
    s = flearn_amd.setup_strategy("normclip", None, tau=3.0, noise_multiplier=1.1, seed=5, sequence=2, output="device")
    assert type(s) is NormClip and (s.tau, s.noise_multiplier, s.seed, s.sequence, s.output) == (3.0, 1.1, 5, 2, "device")
    assert flearn_amd.setup_strategy("normclip", None, tau=3.0).noise_multiplier is None
    for kw in ({"quantile": 0.5, "noise_multiplier": 1.0}, {"tau": math.inf, "noise_multiplier": 1.0},
               {"tau": 1.0, "noise_multiplier": -1.0}, {"tau": 1.0, "noise_multiplier": math.nan},
               {"tau": 1.0, "noise_multiplier": math.inf}, {"tau": 1.0, "noise_multiplier": "2"},
               {"tau": 1.0, "noise_multiplier": 1.0, "seed": -1}, {"tau": 1.0, "noise_multiplier": 1.0, "seed": 2 ** 64},
               {"tau": 1.0, "noise_multiplier": 1.0, "sequence": 1.5}):
        with pytest.raises(ValueError):
            NormClip(**kw)
    with pytest.raises(TypeError):
        NormClip(1.0, None, None, "previous", None, "reference", None, None, None, None, 1.0)  # keyword-only
    assert NormClip(quantile=0.5, noise_multiplier=0).quantile == 0.5  # no noise: nothing to refuse
    doc = NormClip.__doc__
    assert "REPEATS THE" in doc and "cryptographic" in doc and "accounting" in doc
    edoc = flearn_amd.aggregator.Aggregator.ensemble_clipped.__doc__
    assert "outside" in edoc and "guarantee" in edoc and "cryptographic" in edoc


def test_a_noised_first_round_needs_init_global():
    """Without init_global the first round would be the plain mean: refused when noise is on, through
    server_exception's route, with nothing queued and the sequence not advanced."""
    from flearn_amd.strategy import NormClip

    s = NormClip(tau=1.0, noise_multiplier=1.0, seed=3)
    s._engine = bare_engine()
    with pytest.raises(SystemExit):
        s.server([{"agg_weight": 1.0, "params": w} for w in uploads(7)], 0)
    assert s.sequence == 0 and s._prev_glob is None
