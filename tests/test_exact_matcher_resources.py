"""The exact all-pairs scans: K1r is the one-centre instantiation (NC = 1, rows finished by RatioOut) of the scan with exclusion discs
(csrc/match_disc.h), which runs its fold on the two tile walks of csrc/match_tile.h; K1 and K1m carry their own text of both walks.
A fold that does not suit the walk shows first as spilled registers: no instantiation of the kernels below may spill or
use scratch, and none may need more than the 256 VGPRs that two workgroups per CU leave a wave.  match_mutual_staged_kernel has 20 B
of scratch per lane (scalar set-up values spilled to VGPR lanes; DESIGN.md 7g has its measured cost): it must not need more.  No
per-kernel VGPR ceiling beyond that: the count may move, the measured time decides.
All of this held before the test was written: it is the guard for the next attempt to move K1 or K1m onto the header's walks, and for
any new fold.  Mechanism and skip rules of tests/test_handover_resources.py: tools/check_kernel_resources.py on the built objects."""
import glob
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# K1r's instantiations of the templates of csrc/match_disc.h, told from K1n's by the template arguments in the mangled name: <C_pad, NC, Out>,
# <NC, Out>, <Out>
K1R = {"match_disc_regb_kernel": r"ILi\d+ELi1ENS_8RatioOutE", "match_disc_staged_kernel": "ILi1ENS_8RatioOutE", "match_disc_merge_kernel": "INS_8RatioOutE"}
CLEAN = ("match_f32_regb_kernel", "match_f32_kernel", "match_mutual_regb_kernel") + tuple(K1R)
MUTUAL_STAGED = "match_mutual_staged_kernel"
MUTUAL_STAGED_SCRATCH = 20               # bytes per lane
INSTANCES = {"match_f32_regb_kernel": 4, "match_mutual_regb_kernel": 4, "match_disc_regb_kernel": 4,         # C_pad 32 / 64 / 128 / 256
             "match_disc_staged_kernel": 1, "match_disc_merge_kernel": 1}


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
    """the kernel's own name inside an Itanium-mangled symbol of namespace oryon, _ZN5oryon<len><name>..., with K1R's template arguments"""
    return re.compile(f"_ZN5oryon{len(name)}{name}" + K1R.get(name, ""))


def test_exact_scan_kernels_do_not_spill():
    rows = _rows()
    seen = {}
    for k in rows:
        for name in CLEAN + (MUTUAL_STAGED,):
            if not _kernel(name).match(k["name"]):
                continue
            seen[name] = seen.get(name, 0) + 1
            print(k["name"], "vgpr", k["vgpr"], "agpr", k["agpr"], "spill", k["spill"], "scratch", k["scratch"])
            assert k["vgpr"] <= 256, f"{k['name']}: {k['vgpr']} VGPRs"
            if name == MUTUAL_STAGED:
                assert k["scratch"] <= MUTUAL_STAGED_SCRATCH, f"{k['name']}: {k['scratch']} B of scratch per lane, {MUTUAL_STAGED_SCRATCH} allowed"
            else:
                assert k["scratch"] == 0 and k["spill"] == 0, f"{k['name']}: {k['spill']} spilled registers, {k['scratch']} B of scratch per lane"
    assert set(seen) == set(CLEAN + (MUTUAL_STAGED,)), sorted(set(CLEAN + (MUTUAL_STAGED,)) - set(seen))
    for name, n in INSTANCES.items():
        assert seen[name] == n, f"{name}: {seen[name]} instantiations in the objects, {n} widths"
