"""The KNN scan's kernels keep their register budget: read from the device assembly, no GPU needed (tools/knn_isa_report.py).

k_knn_consume runs 16 waves a CU, four a SIMD: 128 vector registers each is all the register file gives, and a 129th halves the occupancy.
Its 16 bytes of scratch (and the seed kernel's none) lie outside the block loop; more would mean a spill moved into it."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("knn_isa_report", os.path.join(ROOT, "tools", "knn_isa_report.py"))
knn_isa_report = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(knn_isa_report)

pytestmark = pytest.mark.skipif(knn_isa_report.find_hipcc() is None, reason="hipcc is not installed")


@pytest.fixture(scope="module")
def isa():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "knn_isa_report.py"), "--ht", "5", "--hq", "4", "--td", "0", "--kernel", "consume",
                          "--kernel", "seed", "--json"], check=True, capture_output=True, text=True).stdout
    res = json.loads(out.strip().splitlines()[-1])
    print(res)
    return res


def test_consume_registers_and_scratch(isa):
    c = isa["consume"]
    assert c["instantiation"] == "k_knn_consume<5, 4, false, false>"
    assert c["next_free_vgpr"] <= 128
    assert c["private_segment_fixed_size"] <= 16  # what the kernel had before its epilogue worked on the mask of minima


def test_seed_scratch(isa):
    s = isa["seed"]
    assert s["instantiation"] == "k_knn_seed<5, 4, false, false>"
    assert s["private_segment_fixed_size"] <= 0  # the seed kernel never spilled
    assert s["next_free_vgpr"] <= 128  # (four workgroups of eight waves a CU by its launch bounds)


def test_report_finds_both_paths(isa):
    """the counts are reported, not bounded (DESIGN 18 states them); they must be there and plausible for the tool to be of use"""
    for k in ("consume", "seed"):
        assert isa[k]["first_look"] >= 8 and isa[k]["exact"] > 0
