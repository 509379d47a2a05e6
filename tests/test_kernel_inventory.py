"""Host-only: the reduce kernel instantiations in the built library, against the case table of
tests/test_gpu_instantiations.py (tests/instantiation_cases.py).

Every `reduce_kernel_*` instantiation the library ships is listed from its symbols; the per-family
counts are pinned, and for every family but the float16 one (tests/test_gpu_half.py) the set of
shipped instantiations must EQUAL the set the case table claims to launch: a kernel added to the
dispatch without a case fails here, and so does a case naming a kernel that is not shipped.  The
GPU matrix then proves each claim (the launch record names the target, results bit-equal to the
oracle).  A missing library, object file or symbol tool is a failure, not a skip."""
import re
import shutil
import subprocess
from collections import Counter
from pathlib import Path

from flearn_amd import _build
from flearn_amd import _native as na
from instantiation_cases import COVERED, FAMILY_COUNTS, TARGETS

KERNEL = re.compile(r"reduce_kernel_[a-z0-9_]+<")


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


def normalise(symbol_line):
    """'... void fa::reduce_kernel_rows<fa::AccF32, float, 0, 1, 16, 4, true>(float const*, ...)'
    -> 'reduce_kernel_rows<AccF32,float,0,1,16,4,true>': the template-id from the family name to
    its closing bracket (the argument list and return type dropped), without `fa::` and whitespace.
    None for a line that names no kernel instantiation."""
    m = KERNEL.search(symbol_line)
    if not m:
        return None
    depth, i = 0, m.end() - 1
    while i < len(symbol_line):
        depth += {"<": 1, ">": -1}.get(symbol_line[i], 0)
        if depth == 0:
            break
        i += 1
    assert depth == 0, symbol_line
    return re.sub(r"\s+", "", symbol_line[m.start() : i + 1].replace("fa::", ""))


def shipped_instantiations():
    objs = [_build.object_of(src) for src in _build.SOURCES]  # build_native leaves them beside the library
    binaries = objs if all(o.exists() for o in objs) else [na.LIB_PATH]
    for binary in binaries:
        assert binary.exists(), f"{binary} not built: run __graft_entry__.build()"
    out = subprocess.run(symbol_lister() + [str(b) for b in binaries], capture_output=True, text=True, check=True).stdout
    # the host stub (__device_stub__...) and the kernel handle demangle to the same template-id
    return {n for n in map(normalise, out.splitlines()) if n}


def family(name):
    return name[len("reduce_kernel_") : name.index("<")]


def test_normalise():
    line = ("0000000000000000 W void fa::reduce_kernel_rowmajor<fa::AccF32, double, 1, 16, 1, 4, 3, true, 4, false, "
            "true>(float const*, long, int, fa::AccF32::w_t const*, long, long, fa::Epi<double>)")
    assert normalise(line) == "reduce_kernel_rowmajor<AccF32,double,1,16,1,4,3,true,4,false,true>"
    stub = line.replace("fa::reduce_kernel", "fa::__device_stub__reduce_kernel")
    assert normalise(stub) == normalise(line)
    assert normalise("0000 T fa_reduce_f32") is None


def test_family_counts():
    got = Counter(family(n) for n in shipped_instantiations())
    assert dict(got) == FAMILY_COUNTS, got


def test_every_shipped_kernel_has_a_case_and_every_case_a_kernel():
    shipped = {n for n in shipped_instantiations() if family(n) in COVERED}
    assert len(shipped) == sum(FAMILY_COUNTS[f] for f in COVERED)
    without_case = sorted(shipped - TARGETS)
    not_shipped = sorted(TARGETS - shipped)
    assert not without_case and not not_shipped, (
        f"{len(without_case)} shipped kernels no case launches: {without_case[:6]}; "
        f"{len(not_shipped)} cases name kernels that are not shipped: {not_shipped[:6]}")
