"""The compiled shape of k_head_stream_sample, the sampling form of the head kernel (tools/head_isa.py; no GPU, needs
hipcc).  Like the default kernels it must fit two workgroups per CU: no scratch, no spills, at most 128 registers and
at most 80 KB of LDS.  Nothing else about its assembly is inspected."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import head_isa  # noqa: E402

pytestmark = pytest.mark.skipif(head_isa.find_hipcc() is None, reason="hipcc is not installed")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("head_sample_isa") / "ofx_head.s")
    head_isa.build_asm(path)
    return open(path).read()


@pytest.mark.parametrize("lp", [0, 1, 2])
def test_two_workgroups_per_cu(asm, lp):
    r = head_isa.report(asm, "_Z20k_head_stream_sampleILi%dEEv11HeadParams2" % lp)
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, r
    assert r["vgprs"] + r["agprs"] <= 128, r
    assert r["lds_bytes"] <= 80 * 1024, r
