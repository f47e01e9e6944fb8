"""The kernels the default-route cascade's sub-bands added to the cfg2 step keep their working set in registers: the 4-wave windowed
screen at every live k-step count and the settle pass (the mechanism and skip rules of test_hot_kernels_do_not_spill:
tools/check_kernel_resources.py on the built objects)."""
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sub_band_kernels_do_not_spill():
    if not glob.glob(os.path.join(ROOT, "oryon_amd", "csrc", "*.o")):
        pytest.skip("objects not built in this tree")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as ckr
    rows = ckr.report()
    if not rows:
        pytest.skip("LLVM object tools not available")
    hot = ("match_mx6_screen_w4_win_kernelILi256ELi4ELi1E", "match_mx6_screen_w4_win_kernelILi256ELi4ELi2E",
           "match_mx6_screen_w4_win_kernelILi256ELi4ELi4E", "match_dc_settle_rows_kernel")
    seen = set()
    for k in rows:
        for h in hot:
            if h in k["name"]:
                seen.add(h)
                assert k["scratch"] == 0, f"{k['name']}: {k['spill']} spilled registers, {k['scratch']} B of scratch per lane"
    assert seen == set(hot), sorted(set(hot) - seen)
