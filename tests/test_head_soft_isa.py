"""The compiled shape of k_head_stream_soft, the soft (log-sum-exp) form of the head kernel (tools/head_isa.py; no GPU,
needs hipcc).  Like the default kernels it must fit two workgroups per CU: no scratch, no spills, at most 128 registers
and at most 80 KB of LDS.  Nothing else about its assembly is inspected."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import head_isa  # noqa: E402

pytestmark = pytest.mark.skipif(head_isa.find_hipcc() is None, reason="hipcc is not installed")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("head_soft_isa") / "ofx_head.s")
    head_isa.build_asm(path)
    return open(path).read()


@pytest.mark.parametrize("extra", [0, 1])
def test_two_workgroups_per_cu(asm, extra):
    r = head_isa.report(asm, "_Z18k_head_stream_softILb%dEEv11HeadParams2" % extra)
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, r
    assert r["vgprs"] + r["agprs"] <= 128, r
    assert r["lds_bytes"] <= 80 * 1024, r
