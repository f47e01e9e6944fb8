"""The kernels of the one-to-many matcher (csrc/match_next.hip, oryon_topk_corrs in csrc/post.hip): the rank scan is the three-centre
instantiation (NC = 3, rows finished by RankOut) of the scan with exclusion discs (csrc/match_disc.h), whose fold runs on the two tile
walks of csrc/match_tile.h; a fold that does not suit a walk shows first as spilled registers.  No instantiation - four
register-resident widths, the staged one, the merge - nor the gather, expansion and rank-1 kernels may spill, use scratch or need more
than the 256 VGPRs that two workgroups per CU leave a wave.
Mechanism and skip rules of tests/test_exact_matcher_resources.py: tools/check_kernel_resources.py on the built objects."""
import glob
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# K1n's instantiations of the templates of csrc/match_disc.h, told from K1r's by the template arguments in the mangled name: <C_pad, NC, Out>,
# <NC, Out>, <Out>
K1N = {"match_disc_regb_kernel": r"ILi\d+ELi3ENS_7RankOutE", "match_disc_staged_kernel": "ILi3ENS_7RankOutE", "match_disc_merge_kernel": "INS_7RankOutE"}
CLEAN = tuple(K1N) + ("topk_gather_kernel", "topk_expand_kernel", "topk_rank1_kernel")
INSTANCES = {"match_disc_regb_kernel": 4, "match_disc_staged_kernel": 1, "match_disc_merge_kernel": 1,       # C_pad 32 / 64 / 128 / 256
             "topk_expand_kernel": 1}


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
    """the kernel's own name inside an Itanium-mangled symbol of namespace oryon, _ZN5oryon<len><name>..., with K1N's template arguments"""
    return re.compile(f"_ZN5oryon{len(name)}{name}" + K1N.get(name, ""))


def test_topk_kernels_do_not_spill():
    rows = _rows()
    seen = {}
    for k in rows:
        for name in CLEAN:
            if not _kernel(name).match(k["name"]):
                continue
            seen[name] = seen.get(name, 0) + 1
            print(k["name"], "vgpr", k["vgpr"], "agpr", k["agpr"], "spill", k["spill"], "scratch", k["scratch"])
            assert k["vgpr"] <= 256, f"{k['name']}: {k['vgpr']} VGPRs"
            assert k["scratch"] == 0 and k["spill"] == 0, f"{k['name']}: {k['spill']} spilled registers, {k['scratch']} B of scratch per lane"
    assert set(seen) == set(CLEAN), sorted(set(CLEAN) - set(seen))
    for name, n in INSTANCES.items():
        assert seen[name] == n, f"{name}: {seen[name]} instantiations in the objects, {n} expected"
