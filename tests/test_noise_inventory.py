"""Host-only: the noise kernel in the built library.  It lives in namespace fa::noise, so the counts
tests/test_kernel_inventory.py pins for namespace fa and the set tests/test_clip_inventory.py pins for
fa::clip hold unchanged (both rerun here); fa::noise ships exactly gauss_add_kernel, the name
tests/test_gpu_noise.py finds in fa_last_launch.  A missing library or symbol tool is a failure, not a
skip."""
import re

import test_clip_inventory as ci
import test_kernel_inventory as ki

NOISE_KERNEL = re.compile(r"\bfa::noise::(?:__device_stub__)?([a-z0-9_]*kernel[a-z0-9_]*)([<(])")


def test_spelling():
    line = "0000000000000000 T fa::noise::gauss_add_kernel(float*, long, long, float, unsigned int, unsigned int, unsigned int, unsigned int)"
    assert NOISE_KERNEL.search(line).group(1) == "gauss_add_kernel"
    assert NOISE_KERNEL.search(line.replace("noise::gauss", "noise::__device_stub__gauss")).group(1) == "gauss_add_kernel"
    # invisible to the parents' inventories
    assert ki.normalise(line) is None and not ki.ANY_KERNEL.search(line) and not ci.CLIP_KERNEL.search(line)


def test_the_noise_unit_ships_one_kernel():
    found = {(m.group(1), m.group(2)) for m in map(NOISE_KERNEL.search, ki.symbol_lines()) if m}
    assert found == {("gauss_add_kernel", "(")}  # one plain kernel, no template instantiations


def test_the_parents_counts_still_hold():
    ki.test_family_counts()
    ki.test_unrecorded_kernel_counts()
    ki.test_every_shipped_kernel_has_a_case_and_every_case_a_kernel()
    ci.test_shipped_clip_kernels_are_the_launched_set()
    ci.test_the_parents_counts_still_hold()
