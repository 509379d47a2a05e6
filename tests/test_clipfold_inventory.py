"""Host-only: the streamed clipped round's kernel in the built library.  It lives in namespace
fa::clipfold, so the counts tests/test_kernel_inventory.py pins for namespace fa, the set
tests/test_clip_inventory.py pins for fa::clip and the one tests/test_noise_inventory.py pins for
fa::noise hold unchanged (all rerun here); its instantiations, listed from the library's symbols the
way those files list theirs, must EQUAL tests/clipfold_ref.py's table, which tests/test_gpu_clip_fold.py
launches and finds named by fa_last_launch.  A missing library or symbol tool is a failure, not a skip."""
import re

import clip_ref as cr
import clipfold_ref as cf
import test_clip_inventory as ci
import test_kernel_inventory as ki
import test_noise_inventory as ni

CLIPFOLD_KERNEL = re.compile(r"\bfa::clipfold::(?:__device_stub__)?([a-z0-9_]*kernel[a-z0-9_]*)([<(])")


def clipfold_kernels():
    """(template instantiations, plain kernels) of namespace fa::clipfold, spelled as fa_last_launch does."""
    templates, plain = set(), set()
    for line in ki.symbol_lines():
        m = CLIPFOLD_KERNEL.search(line)
        if not m:
            continue
        if m.group(2) == "<":
            templates.add(ki.template_id(line, m.start(1)).replace("clipfold::", ""))
        else:
            plain.add(m.group(1))
    return templates, plain


def test_spelling():
    line = ("0000000000000000 W void fa::clipfold::clip_fold_kernel<16, 1, 4, true>(float const*, long, int, "
            "float const*, float const*, float const*, float*, long, long)")
    m = CLIPFOLD_KERNEL.search(line)
    assert ki.template_id(line, m.start(1)) == "clip_fold_kernel<16,1,4,true>" == cr.instance(cf.FAMILY, 16)
    stub = line.replace("clipfold::clip_fold", "clipfold::__device_stub__clip_fold")
    assert CLIPFOLD_KERNEL.search(stub).group(1) == "clip_fold_kernel"
    # invisible to the parents' inventories
    assert ki.normalise(line) is None and not ki.ANY_KERNEL.search(line)
    assert not ci.CLIP_KERNEL.search(line) and not ni.NOISE_KERNEL.search(line)
    assert not any(re.search(fam, t) for t in cf.TARGETS for fam in ki.RECORDED)


def test_shipped_clipfold_kernels_are_the_launched_set():
    templates, plain = clipfold_kernels()
    assert templates == cf.TARGETS, (sorted(templates - cf.TARGETS), sorted(cf.TARGETS - templates))
    assert plain == set()
    assert len(cf.TARGETS) == len(cf.VS) == 5  # one per piece width; open / continue is a run-time test


def test_the_parents_counts_still_hold():
    ki.test_family_counts()
    ki.test_unrecorded_kernel_counts()
    ki.test_every_shipped_kernel_has_a_case_and_every_case_a_kernel()
    ci.test_shipped_clip_kernels_are_the_launched_set()
    ni.test_the_noise_unit_ships_one_kernel()
