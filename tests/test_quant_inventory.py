"""Host-only: the quantized round's kernel in the built library.  It lives in namespace fa::quant, so
the counts tests/test_kernel_inventory.py pins for namespace fa, the sets tests/test_clip_inventory.py
and tests/test_clipfold_inventory.py pin for fa::clip and fa::clipfold and the one
tests/test_noise_inventory.py pins for fa::noise hold unchanged (all rerun here); its instantiations,
listed from the library's symbols the way those files list theirs, must EQUAL tests/quant_ref.py's
table, which tests/test_gpu_deq_fold.py launches and finds named by fa_last_launch.  A missing library
or symbol tool is a failure, not a skip."""
import re

import quant_ref as qr
import test_clip_inventory as ci
import test_clipfold_inventory as cfi
import test_kernel_inventory as ki
import test_noise_inventory as ni

QUANT_KERNEL = re.compile(r"\bfa::quant::(?:__device_stub__)?([a-z0-9_]*kernel[a-z0-9_]*)([<(])")


def quant_kernels():
    """(template instantiations, plain kernels) of namespace fa::quant, spelled as fa_last_launch does."""
    templates, plain = set(), set()
    for line in ki.symbol_lines():
        m = QUANT_KERNEL.search(line)
        if not m:
            continue
        if m.group(2) == "<":
            templates.add(ki.template_id(line, m.start(1)).replace("quant::", ""))
        else:
            plain.add(m.group(1))
    return templates, plain


def test_spelling():
    line = ("0000000000000000 W void fa::quant::deq_fold_kernel<2, 8, 4, true>(signed char const*, long, int, "
            "float const*, long, float const*, float const*, float const*, float*, long, long)")
    m = QUANT_KERNEL.search(line)
    assert ki.template_id(line, m.start(1)) == "deq_fold_kernel<2,8,4,true>" == qr.instance(2)
    stub = line.replace("quant::deq_fold", "quant::__device_stub__deq_fold")
    assert QUANT_KERNEL.search(stub).group(1) == "deq_fold_kernel"
    # invisible to the parents' inventories
    assert ki.normalise(line) is None and not ki.ANY_KERNEL.search(line)
    assert not ci.CLIP_KERNEL.search(line) and not ni.NOISE_KERNEL.search(line) and not cfi.CLIPFOLD_KERNEL.search(line)
    assert not any(re.search(fam, t) for t in qr.TARGETS for fam in ki.RECORDED)


def test_shipped_quant_kernels_are_the_launched_set():
    templates, plain = quant_kernels()
    assert templates == qr.TARGETS, (sorted(templates - qr.TARGETS), sorted(qr.TARGETS - templates))
    assert plain == set()
    assert len(qr.TARGETS) == len(qr.VS) == 2  # one per piece width; centre and open / continue are run-time tests


def test_the_parents_counts_still_hold():
    ki.test_family_counts()
    ki.test_unrecorded_kernel_counts()
    ki.test_every_shipped_kernel_has_a_case_and_every_case_a_kernel()
    ci.test_shipped_clip_kernels_are_the_launched_set()
    cfi.test_shipped_clipfold_kernels_are_the_launched_set()
    ni.test_the_noise_unit_ships_one_kernel()
