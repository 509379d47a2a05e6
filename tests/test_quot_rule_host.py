"""Host-only: which weight sums take the epilogues' reciprocal quotient (fa::recip_quot_exact,
flearn_amd/csrc/fa_geometry.hpp; tests/quot_rule_probe.cpp is compiled against that header alone).

The rule is the proof's: finite and non-zero, 2^-100 <= |d| <= 2^100, and at most 27
significant bits.  Everything else keeps the IEEE divide."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "flearn_amd" / "csrc"


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    exe = tmp_path_factory.mktemp("quot_rule") / "quot_rule_probe"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(CSRC), "-I", str(REPO / "include"),
                    str(REPO / "tests" / "quot_rule_probe.cpp"), "-o", str(exe)], check=True)

    def ask(denoms):
        text = "".join(struct.pack(">d", float(d)).hex() + "\n" for d in denoms)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == len(denoms)
        return [o == "1" for o in out]

    return ask


def in_python(d):
    """The rule restated: the significand as an integer has at most 27 bits."""
    d = float(d)
    if not np.isfinite(d) or d == 0.0 or not 2.0**-100 <= abs(d) <= 2.0**100:
        return False
    m, _ = np.frexp(abs(d))  # m in [0.5, 1): m * 2^27 is an integer exactly when 27 bits suffice
    return float(m) * 2.0**27 == int(float(m) * 2.0**27)


TAKES = [100.0, 3.0, 2.0**26 + 1, -7.0, 1.0, -100.0, 1000.0, 2.0**27, 2.0**27 - 1, 2.0**100, -(2.0**100), 2.0**-100,
         (2.0**27 - 1) * 2.0**-126, (2.0**27 - 1) * 2.0**73]
KEEPS_IEEE = [2.0**27 + 1, 0.001, float("inf"), float("-inf"), float("nan"), 0.0, -0.0, 2.0**101, 2.0**-101,
              -(2.0**101), 1e30 * 1e10, 5e-324, 2.0**-1022, 1.0 / 3.0, 0.1, 2.0**100 * (1 + 2.0**-26),
              np.nextafter(2.0**100, np.inf), np.nextafter(2.0**-100, 0.0), 2.0**53 + 2.0, 1.0 + 2.0**-27]


def test_the_issue_cases(rule):
    assert rule([100.0, 3.0, 2.0**26 + 1]) == [True, True, True]  # 2^26 + 1: the last odd integer that qualifies
    assert rule([2.0**27 + 1]) == [False]  # 28 significant bits
    assert rule([0.001, float("inf"), float("-inf"), float("nan"), 0.0]) == [False] * 5
    assert rule([2.0**101, 2.0**-101]) == [False, False]


def test_takes_and_keeps(rule):
    assert rule(TAKES) == [True] * len(TAKES)
    assert rule(KEEPS_IEEE) == [False] * len(KEEPS_IEEE)
    assert all(in_python(d) for d in TAKES) and not any(in_python(d) for d in KEEPS_IEEE)


def test_rule_against_its_restatement(rule):
    """Random bit patterns around the three edges: the mantissa's low bits, the exponent range."""
    rng = np.random.default_rng(28)
    n = 4000
    exp = rng.choice([1023 - 102, 1023 - 101, 1023 - 100, 1023 - 99, 1023, 1023 + 26, 1023 + 99, 1023 + 100,
                      1023 + 101, 0, 2047], n).astype(np.uint64)
    keep = rng.integers(20, 33, n).astype(np.uint64)  # mantissa bits kept from the top: 26 is the last that passes
    mant = rng.integers(0, 2**52, n, dtype=np.uint64) >> (np.uint64(52) - keep) << (np.uint64(52) - keep)
    sign = rng.integers(0, 2, n).astype(np.uint64)
    d = ((sign << np.uint64(63)) | (exp << np.uint64(52)) | mant).view(np.float64)
    got = rule(list(d))
    want = [in_python(x) for x in d]
    assert got == want
    assert 0.2 < np.mean(want) < 0.8  # both answers are exercised


def test_weight_sums_of_flearn_rounds_qualify(rule):
    """Sample counts and unit weights: every integer sum up to 2^27 has at most 27 significant bits."""
    sums = [float(s) for s in (1, 2, 10, 100, 600, 60_000, 2**27)] + [float(np.sum(np.full(100, 1.0)))]
    assert rule(sums) == [True] * len(sums)
