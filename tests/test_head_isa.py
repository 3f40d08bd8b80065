"""The compiled shape of k_head_stream (tools/head_isa.py; no GPU, needs hipcc).

The kernel's speed hangs on properties of the generated code that no numerical test sees: two workgroups per CU (at
most 128 VGPRs, at most 80 KB of LDS, no scratch) and a consumers' pass whose waits never drain the vector-memory
counter (the stage-A operands and the frame corrections are requested a sub-step ahead; a `vmcnt(0)` in the block of
the stencil means some load is issued in front of its use again and the HBM latency is exposed in every sub-step).
A refactor that compiled to another schedule once cost 1.4 ms unnoticed for three commits.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import head_isa  # noqa: E402

pytestmark = pytest.mark.skipif(head_isa.find_hipcc() is None, reason="hipcc is not installed")

# (EXTRA, LP): the rollout's forward, the forward that stores the heat map / a probe, and their bf16 / fp16 forms
INSTANCES = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2)]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("head_isa") / "ofx_head.s")
    head_isa.build_asm(path)
    return open(path).read()


@pytest.mark.parametrize("extra,lp", INSTANCES)
def test_two_workgroups_per_cu(asm, extra, lp):
    r = head_isa.report(asm, "_Z13k_head_streamILb%dELi%dEEv11HeadParams2" % (extra, lp))
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, r
    assert r["vgprs"] + r["agprs"] <= 128, r
    assert r["lds_bytes"] <= 80 * 1024, r


@pytest.mark.parametrize("extra,lp", INSTANCES)
def test_consumer_pass_keeps_loads_in_flight(asm, extra, lp):
    r = head_isa.report(asm, "_Z13k_head_streamILb%dELi%dEEv11HeadParams2" % (extra, lp))
    cons, prod = r["loops"]["consumer"], r["loops"]["producer"]
    assert cons is not None and prod is not None, "sub-step loops not found"
    # the loops are the ones meant: the stencil's packed FMAs and stage A's 5 MFMAs; stage B and the 1x1
    assert cons["totals"]["packed"] >= 60 and cons["totals"]["mfma"] == 5, cons["totals"]
    assert prod["totals"]["mfma"] >= 60 and prod["totals"]["packed"] == 0, prod["totals"]
    stencil = [b for b in cons["blocks"] if b["stencil"]]
    assert stencil
    for b in stencil:
        assert not any("vmcnt(0)" in w for w in b["vm_waits"]), (b["block"], b["vm_waits"])


def test_command_line_json():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "head_isa.py"), "--json"], check=True,
                         stdout=subprocess.PIPE, universal_newlines=True).stdout
    r = json.loads(out)
    assert r["kernel"] == "_Z13k_head_streamILb0ELi0EEv11HeadParams2" and r["loops"]["consumer"]["blocks"]
