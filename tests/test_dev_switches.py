"""The development switches of csrc/ (dev_env_int / dev_env_set, read by the development build only) are exactly the ones something
still uses: a test, a tool that is not the record of one round, or README / DESIGN / INTEGRATION.md.  A switch nothing uses fails here
instead of staying in the kernels; retiring one means removing its read and the code only it reached (DESIGN_HISTORY.md lists the
retired ones)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oryon_amd", "csrc")

KEPT = [
    "ORYON_AMB_X3",
    "ORYON_DC_SUB_STATS",
    "ORYON_ENGINE_ABLATE",
    "ORYON_GATHER8_LPR",
    "ORYON_GTC_PPL",
    "ORYON_MX6_VAR",
    "ORYON_PDSC_ATT_SPLITS",
    "ORYON_PDSC_CLOCKS",
    "ORYON_PDSC_FP32_MFMA",
    "ORYON_PDSC_FUSED_HEAD",
    "ORYON_PDSC_ROUTE",
    "ORYON_RESCORE_LANES",
    "ORYON_SCREEN8_ABLATE",
    "ORYON_SCREEN8_VARIANT",
    "ORYON_SCREEN8_WAVES",
]

ROUND_FILE = re.compile(r"^r\d+_")          # tools/r4_*, r5_*, r6_*: records of single rounds, nobody runs them


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _switches_read():
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")):
        names.update(re.findall(r"dev_env_(?:int|set)\(\s*\"([A-Za-z0-9_]+)\"", _read(path)))
    return names


def _supporting_files():
    files = [os.path.join(ROOT, n) for n in ("README.md", "DESIGN.md", "INTEGRATION.md")]
    for dirpath, _, names in os.walk(os.path.join(ROOT, "tests")):
        files += [os.path.join(dirpath, n) for n in names if n.endswith(".py") and os.path.join(dirpath, n) != os.path.abspath(__file__)]
    tools = os.path.join(ROOT, "tools")
    files += [os.path.join(tools, n) for n in os.listdir(tools) if os.path.isfile(os.path.join(tools, n)) and not ROUND_FILE.match(n)]
    return [f for f in files if os.path.isfile(f)]


def test_every_switch_the_sources_read_is_on_the_kept_list():
    assert sorted(_switches_read()) == sorted(KEPT)


def test_every_kept_switch_is_used_by_a_test_a_tool_or_a_document():
    texts = {f: _read(f) for f in _supporting_files()}
    unused = [n for n in KEPT if not any(re.search(rf"\b{n}\b", t) for t in texts.values())]
    assert not unused, f"nothing sets or documents {unused}: retire them (read -> default, and the code only they reached)"
