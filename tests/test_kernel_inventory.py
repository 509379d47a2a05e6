"""Host-only: the kernel instantiations in the built library, against the case table of the GPU
matrices (tests/instantiation_cases.py).

Every instantiation of a kernel family whose launches fa_last_launch reports — the `reduce_kernel_*`
families (the float16 one included), fold_kernel_rows, fold_kernel_elem, fold_finish_kernel,
trim_kernel_rows, trim_kernel_elem and gram_kernel_tile — is listed from the library's symbols; the
per-family counts are pinned, and the set of shipped instantiations must EQUAL the set the case
table claims to launch: a kernel added to the dispatch without a case fails here, and so does a case
naming a kernel that is not shipped.  The GPU tests then prove each claim (the launch record names
the target, results bit-equal to the oracle): tests/test_gpu_instantiations.py,
test_gpu_half_instantiations.py, test_gpu_fold.py, test_gpu_trim.py and test_gpu_gram.py.

Kernels that leave no launch record (apply_kernel, the gather, copy, push, fence and fill kernels,
and gram_finish_kernel, which runs behind the recorded gram_kernel_tile) have their counts pinned
only: nothing names them on the GPU, so there is no claim to compare with.  A missing library,
object file or symbol tool is a failure, not a skip."""
import re
import shutil
import subprocess
from collections import Counter
from pathlib import Path

import pytest

from flearn_amd import _build
from flearn_amd import _native as na
from instantiation_cases import COVERED, FAMILY_COUNTS, TARGETS, UNRECORDED_COUNTS

RECORDED = ("reduce_kernel_[a-z0-9_]+", "fold_kernel_rows", "fold_kernel_elem", "fold_finish_kernel", "trim_kernel_rows",
            "trim_kernel_elem", "gram_kernel_tile")
KERNEL = re.compile(r"(?:%s)<" % "|".join(RECORDED))
# any kernel of namespace fa, a template or not, as a host stub or a kernel handle
ANY_KERNEL = re.compile(r"\bfa::(?:__device_stub__)?([a-z0-9_]*kernel[a-z0-9_]*)[<(]")


def symbol_lister():
    """The command that prints demangled symbols: llvm-nm -C of the ROCm that _build.hipcc()
    belongs to; ROCm installs without llvm-nm carry llvm-readelf, whose --symbols --demangle
    prints the same names; then the system's nm -C (what tests/test_cabi.py reads exports with)."""
    rocm = Path(_build.hipcc()).resolve().parent.parent
    for sub in ("lib/llvm/bin", "llvm/bin", "bin"):
        for tool, args in (("llvm-nm", ["-C"]), ("llvm-readelf", ["--symbols", "--demangle", "--wide"])):
            exe = rocm / sub / tool
            if exe.exists():
                return [str(exe)] + args
    for tool in ("llvm-nm", "nm"):
        if shutil.which(tool):
            return [shutil.which(tool), "-C"]
    raise AssertionError(f"no llvm-nm / llvm-readelf under {rocm} and no nm on PATH")


def template_id(symbol_line, start):
    """The template-id that begins at `start`, up to its closing bracket, without `fa::` and
    whitespace."""
    depth, i = 0, symbol_line.index("<", start)
    while i < len(symbol_line):
        depth += {"<": 1, ">": -1}.get(symbol_line[i], 0)
        if depth == 0:
            break
        i += 1
    assert depth == 0, symbol_line
    return re.sub(r"\s+", "", symbol_line[start : i + 1].replace("fa::", ""))


def normalise(symbol_line):
    """'... void fa::reduce_kernel_rows<fa::AccF32, float, 0, 1, 16, 4, true>(float const*, ...)'
    -> 'reduce_kernel_rows<AccF32,float,0,1,16,4,true>': the template-id from the family name to
    its closing bracket (the argument list and return type dropped), without `fa::` and whitespace.
    None for a line that names no instantiation of a recorded family."""
    m = KERNEL.search(symbol_line)
    return template_id(symbol_line, m.start()) if m else None


def symbol_lines():
    objs = [_build.object_of(src) for src in _build.SOURCES]  # build_native leaves them beside the library
    binaries = objs if all(o.exists() for o in objs) else [na.LIB_PATH]
    for binary in binaries:
        assert binary.exists(), f"{binary} not built: run __graft_entry__.build()"
    return subprocess.run(symbol_lister() + [str(b) for b in binaries], capture_output=True, text=True,
                          check=True).stdout.splitlines()


def shipped_instantiations():
    # the host stub (__device_stub__...) and the kernel handle demangle to the same template-id
    return {n for n in map(normalise, symbol_lines()) if n}


def family(name):
    name = name[: name.index("<")]
    return name[len("reduce_kernel_"):] if name.startswith("reduce_kernel_") else name


def test_normalise():
    line = ("0000000000000000 W void fa::reduce_kernel_rowmajor<fa::AccF32, double, 1, 16, 1, 4, 3, true, 4, false, "
            "true>(float const*, long, int, fa::AccF32::w_t const*, long, long, fa::Epi<double>)")
    assert normalise(line) == "reduce_kernel_rowmajor<AccF32,double,1,16,1,4,3,true,4,false,true>"
    stub = line.replace("fa::reduce_kernel", "fa::__device_stub__reduce_kernel")
    assert normalise(stub) == normalise(line)
    assert normalise("0000 T fa_reduce_f32") is None


# one symbol line per recorded family beside the one above, as llvm-nm -C / llvm-readelf print them
SPELLINGS = {
    "rows_h16": ("0000000000000000 W void fa::reduce_kernel_rows_h16<fa::AccH16Pk, 2, 16, 1, 4, true>(unsigned short const*, "
                 "long, int, fa::AccH16Pk::w_t const*, long, long, fa::EpiH16)",
                 "reduce_kernel_rows_h16<AccH16Pk,2,16,1,4,true>"),
    "fold_kernel_rows": ("   636: 0000000000000000     8 OBJECT  WEAK   DEFAULT   457 void fa::fold_kernel_rows<fa::AccF32W64, "
                         "1, 16, 4, true>(float const*, long, int, fa::AccF32W64::w_t const*, fa::AccF32W64::acc_t const*, "
                         "fa::AccF32W64::acc_t*, long, long)",
                         "fold_kernel_rows<AccF32W64,1,16,4,true>"),
    "fold_kernel_elem": ("0000000000000000 W void fa::fold_kernel_elem<fa::AccI64>(fa::AccI64::x_t const*, long, int, "
                         "fa::AccI64::w_t const*, fa::AccI64::acc_t const*, fa::AccI64::acc_t*, long, long)",
                         "fold_kernel_elem<AccI64>"),
    "fold_finish_kernel": ("0000000000000000 W void fa::fold_finish_kernel<long, double, 0>(long const*, long, fa::Epi<double>)",
                           "fold_finish_kernel<long,double,0>"),
    "trim_kernel_rows": ("0000000000000000 W void fa::trim_kernel_rows<128, 4, true>(float const*, long, int, int, float*, "
                         "long, long)",
                         "trim_kernel_rows<128,4,true>"),
    "trim_kernel_elem": ("0000000000000000 W void fa::trim_kernel_elem<long>(long const*, long, int, int, long*, long, long)",
                         "trim_kernel_elem<long>"),
    "gram_kernel_tile": ("0000000000000000 W void fa::gram_kernel_tile<96, false, true>(float const*, long, int, "
                         "float const*, long, long, long, float*)",
                         "gram_kernel_tile<96,false,true>"),
}


@pytest.mark.parametrize("fam", sorted(SPELLINGS))
def test_normalise_family_spelling(fam):
    line, want = SPELLINGS[fam]
    name = want[: want.index("<")]
    assert normalise(line) == want and family(want) == fam
    assert normalise(line.replace(f"fa::{name}", f"fa::__device_stub__{name}")) == want
    assert want in TARGETS  # the table spells its targets the same way


def test_normalise_skips_unrecorded_kernels_and_functions():
    assert set(SPELLINGS) | {"rowmajor"} <= set(FAMILY_COUNTS)
    assert normalise("0000 T fa::gram_finish_kernel(float const*, long, int, int, double*)") is None
    assert normalise("0000 W void fa::apply_kernel<double, 1>(double const*, long, fa::Epi<double>)") is None
    assert normalise("0000 W fa::host::make_kernel_name(char const*, std::string const&)") is None


def test_family_counts():
    got = Counter(family(n) for n in shipped_instantiations())
    assert dict(got) == FAMILY_COUNTS, got


def test_unrecorded_kernel_counts():
    """Every other kernel of namespace fa, by name and (for templates) template-id: counts only."""
    seen = set()
    for line in symbol_lines():
        m = ANY_KERNEL.search(line)
        if m and not KERNEL.search(line):
            start = m.start(1)
            seen.add(template_id(line, start) if line[m.end() - 1] == "<" else m.group(1))
    got = Counter(n.split("<")[0] for n in seen)
    assert dict(got) == UNRECORDED_COUNTS, got


def test_every_shipped_kernel_has_a_case_and_every_case_a_kernel():
    assert set(COVERED) == set(FAMILY_COUNTS)  # no recorded family is left out
    shipped = {n for n in shipped_instantiations() if family(n) in COVERED}
    without_case = sorted(shipped - TARGETS)
    not_shipped = sorted(TARGETS - shipped)
    assert not without_case and not not_shipped, (
        f"{len(without_case)} shipped kernels no case launches: {without_case[:6]}; "
        f"{len(not_shipped)} cases name kernels that are not shipped: {not_shipped[:6]}")
    assert len(shipped) == sum(FAMILY_COUNTS[f] for f in COVERED)
