"""The kernels of the one-to-many matcher (csrc/match_next.hip, oryon_topk_corrs in csrc/post.hip): the rank scan is K1r's fold with
three centres per anchor column on the two tile walks of csrc/match_tile.h; a fold that does not suit a walk shows first as spilled
registers.  No instantiation - four register-resident widths, the staged one - nor the gather, expansion and merge
kernels may spill, use scratch or need more than the 256 VGPRs that two workgroups per CU leave a wave.
Mechanism and skip rules of tests/test_exact_matcher_resources.py: tools/check_kernel_resources.py on the built objects."""
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CLEAN = ("match_next_regb_kernel", "match_next_staged_kernel", "match_next_merge_kernel", "topk_gather_kernel", "topk_expand_kernel",
         "topk_rank1_kernel")
INSTANCES = {"match_next_regb_kernel": 4, "match_next_staged_kernel": 1, "topk_expand_kernel": 1}       # C_pad 32 / 64 / 128 / 256


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


def test_topk_kernels_do_not_spill():
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
    for name, n in INSTANCES.items():
        assert seen[name] == n, f"{name}: {seen[name]} instantiations in the objects, {n} expected"
