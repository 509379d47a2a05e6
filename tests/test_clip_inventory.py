"""Host-only: the norm-clipping kernels in the built library.  They live in namespace fa::clip, so
the counts tests/test_kernel_inventory.py pins for namespace fa hold unchanged (rerun here); their
instantiations, listed from the library's symbols the way that file lists its own, must EQUAL the set
tests/clip_ref.py's table claims and tests/test_gpu_rownorm.py / test_gpu_clip_sum.py launch and find
named by fa_last_launch.  A missing library or symbol tool is a failure, not a skip."""
import re

import clip_ref as cr
import test_kernel_inventory as ki

CLIP_KERNEL = re.compile(r"\bfa::clip::(?:__device_stub__)?([a-z0-9_]*kernel[a-z0-9_]*)([<(])")


def clip_kernels():
    """(template instantiations, plain kernels) of namespace fa::clip, spelled as fa_last_launch does."""
    templates, plain = set(), set()
    for line in ki.symbol_lines():
        m = CLIP_KERNEL.search(line)
        if not m:
            continue
        if m.group(2) == "<":
            templates.add(ki.template_id(line, m.start(1)).replace("clip::", ""))
        else:
            plain.add(m.group(1))
    return templates, plain


def test_spelling():
    line = ("0000000000000000 W void fa::clip::rownorm_kernel<16, 1, 4, true>(float const*, long, int, float const*, "
            "long, long, long, float*)")
    m = CLIP_KERNEL.search(line)
    assert ki.template_id(line, m.start(1)) == "rownorm_kernel<16,1,4,true>" == cr.instance("rownorm_kernel", 16)
    assert CLIP_KERNEL.search(line.replace("clip::rownorm", "clip::__device_stub__rownorm")).group(1) == "rownorm_kernel"
    assert ki.normalise(line) is None and not ki.ANY_KERNEL.search(line)  # invisible to the parent's inventory
    assert not any(re.search(fam, t) for t in cr.TARGETS | cr.UNRECORDED for fam in ki.RECORDED)


def test_shipped_clip_kernels_are_the_launched_set():
    templates, plain = clip_kernels()
    assert templates == cr.TARGETS, (sorted(templates - cr.TARGETS), sorted(cr.TARGETS - templates))
    assert plain == cr.UNRECORDED


def test_the_parents_counts_still_hold():
    ki.test_family_counts()
    ki.test_unrecorded_kernel_counts()
    ki.test_every_shipped_kernel_has_a_case_and_every_case_a_kernel()
