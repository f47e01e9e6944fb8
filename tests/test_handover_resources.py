"""The index-fed 4-wave screen (match_mx6_screen_w4_list_kernel: the cascades' probe, open-row and sampled-row passes read their rows in
place through a list) keeps the register allocation of the kernel it replaced on those passes - the tile loop is the full screen's, only
the prologue's row address differs: no scratch, and no more VGPRs than match_mx6_screen_w4_kernel<256, 4, KL> had over dense panels
(142 / 182 / 251 at KL = 1 / 2 / 4 in the objects of the commit before; DESIGN quotes 141 / 182 / 250 for the windowed twin).  The 8-wave
instantiations are what they were.  Mechanism and skip rules of tests/test_cascade_kernel_resources.py: tools/check_kernel_resources.py on
the built objects."""
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LIST_VGPRS = {"match_mx6_screen_w4_list_kernelILi1E": 141, "match_mx6_screen_w4_list_kernelILi2E": 182, "match_mx6_screen_w4_list_kernelILi4E": 250}
# the 8-wave kernels of the full screen and of the hard route's windowed / gated launches, as built before the list kernel existed
EIGHT_WAVE_VGPRS = {"match_mx6_screen_w4_kernelILi256ELi8ELi1E": 138, "match_mx6_screen_w4_kernelILi256ELi8ELi2E": 174,
                    "match_mx6_screen_w4_kernelILi256ELi8ELi4E": 254, "match_mx6_screen_w4_win_kernelILi256ELi8ELi1E": 137,
                    "match_mx6_screen_w4_win_kernelILi256ELi8ELi2E": 173, "match_mx6_screen_w4_win_kernelILi256ELi8ELi4E": 253}


def _rows():
    if not glob.glob(os.path.join(ROOT, "oryon_amd", "csrc", "*.o")):
        pytest.skip("objects not built in this tree")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as ckr
    rows = ckr.report()
    if not rows:
        pytest.skip("LLVM object tools not available")
    return rows


def _check(rows, bars):
    seen = set()
    for k in rows:
        for h, vgprs in bars.items():
            if h in k["name"]:
                seen.add(h)
                print(k["name"], "vgpr", k["vgpr"], "spill", k["spill"], "scratch", k["scratch"])
                assert k["scratch"] == 0 and k["spill"] == 0, f"{k['name']}: {k['spill']} spilled registers, {k['scratch']} B of scratch per lane"
                assert k["vgpr"] <= vgprs, f"{k['name']}: {k['vgpr']} VGPRs, {vgprs} before"
    assert seen == set(bars), sorted(set(bars) - seen)


def test_list_screen_keeps_the_dense_panel_kernels_registers():
    _check(_rows(), LIST_VGPRS)


def test_eight_wave_screens_are_not_moved():
    _check(_rows(), EIGHT_WAVE_VGPRS)
