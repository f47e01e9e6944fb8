"""The kernels of the sub-pixel refinement (csrc/match_subpix.hip): the fit keeps nineteen float64 sums per lane through a fully
unrolled stencil and the lift inlines two bilinear reads; neither may spill, use scratch or need more than 256 VGPRs.
Mechanism and skip rules of tests/test_topk_kernel_resources.py: tools/check_kernel_resources.py on the built objects."""
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CLEAN = ("subpix_fit_kernel", "subpix_count_kernel", "lift_pairs_subpix_kernel")


def _rows():
    if not glob.glob(os.path.join(ROOT, "oryon_amd", "csrc", "*.o")):
        pytest.skip("objects not built in this tree")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as ckr
    rows = ckr.report()
    if not rows:
        pytest.skip("LLVM object tools not available")
    return rows


def _kernel(name):
    """the kernel's own name inside an Itanium-mangled symbol of namespace oryon: _ZN5oryon<len><name>..."""
    return f"_ZN5oryon{len(name)}{name}"


def test_subpix_kernels_do_not_spill():
    rows = _rows()
    seen = {}
    for k in rows:
        for name in CLEAN:
            if not k["name"].startswith(_kernel(name)):
                continue
            seen[name] = seen.get(name, 0) + 1
            print(k["name"], "vgpr", k["vgpr"], "agpr", k["agpr"], "spill", k["spill"], "scratch", k["scratch"])
            assert k["vgpr"] <= 256, f"{k['name']}: {k['vgpr']} VGPRs"
            assert k["scratch"] == 0 and k["spill"] == 0, f"{k['name']}: {k['spill']} spilled registers, {k['scratch']} B of scratch per lane"
    assert set(seen) == set(CLEAN), sorted(set(CLEAN) - set(seen))
    assert all(n == 1 for n in seen.values()), seen
