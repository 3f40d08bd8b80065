"""Instruction budget of k_head_stream's two sub-step loops, from the compiler's assembly (no GPU needed).

Builds ofighters_amd/csrc/ofx_head.hip to gfx950 assembly with the Makefile's FLAGS + POLICY_FLAGS (or reads a .s file
given with --asm), finds the producers' and the consumers' sub-step loop of one instantiation of k_head_stream and prints,
per basic block, the counts of MFMA / packed VALU / other VALU / LDS / global / scalar-memory instructions and every
s_waitcnt that has a vmcnt field, plus the kernel's register, LDS and scratch figures.

    python tools/head_isa.py                 # k_head_stream<false, 0>, the rollout's forward
    python tools/head_isa.py --extra 1       # k_head_stream<true, 0>
    python tools/head_isa.py --json          # the same as one JSON object (tests/test_head_isa.py reads this)

The consumers' loop is the loop that holds v_pk_fma_f32 (the stencil), the producers' loop the other one with the
MFMAs of stage B (16x16x4 f32 and the 4x4x1 of the 1x1).  A loop is the set of basic blocks on a cycle of the control-flow graph through that block.
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofighters_amd", "csrc")


def make_var(text, name):
    m = re.search(r"^%s\s*\??=\s*(.*)$" % re.escape(name), text, re.M)
    return m.group(1).strip() if m else ""


def find_hipcc():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for c in (os.environ.get("HIPCC"), make_var(mk, "HIPCC"), shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def build_asm(out, extra=()):
    """hipcc -S --cuda-device-only with the flags ofx_head.o is built with."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    arch = make_var(mk, "ARCH") or "gfx950"
    flags = make_var(mk, "FLAGS").replace("$(ARCH)", arch).split() + make_var(mk, "POLICY_FLAGS").split()
    cmd = [find_hipcc()] + flags + list(extra) + ["-S", "--cuda-device-only", "ofx_head.hip", "-o", out]
    subprocess.run(cmd, cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_pk_"):
        return "packed"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "global"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    return "other"


KINDS = ("mfma", "packed", "valu", "lds", "global", "smem")


def parse_kernel(text, kernel):
    a = text.index("\n" + kernel + ":")
    b = text.index(".Lfunc_end", a)
    blocks, cur = [], {"name": "entry", "ins": []}
    for line in text[a:b].split("\n")[2:]:
        t = line.split(";")[0].strip()
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            blocks.append(cur)
            cur = {"name": m.group(1), "ins": []}
            continue
        if not t or t.startswith(".") or re.match(r"^[\w.$]+:", t):
            continue
        cur["ins"].append(t)
    blocks.append(cur)
    index = {blk["name"]: i for i, blk in enumerate(blocks)}
    succ = []
    for i, blk in enumerate(blocks):
        out, fall = set(), True
        for t in blk["ins"]:
            m = re.match(r"^s_(c?)branch\w*\s+(\.LBB\d+_\d+)", t)
            if m:
                out.add(index[m.group(2)])
                fall = bool(m.group(1))
            elif t.startswith("s_endpgm"):
                fall = False
            else:
                fall = True
        if fall and i + 1 < len(blocks):
            out.add(i + 1)
        succ.append(sorted(out))
    for blk in blocks:
        c = dict.fromkeys(KINDS, 0)
        for t in blk["ins"]:
            k = classify(t.split()[0])
            if k in c:
                c[k] += 1
        blk["counts"] = c
        blk["n"] = len(blk["ins"])
        blk["vm_waits"] = [t for t in blk["ins"] if t.startswith("s_waitcnt") and "vmcnt" in t]
        blk["pk_fma"] = sum(t.startswith("v_pk_fma_f32") for t in blk["ins"])
    return blocks, succ


def reach(succ, start):
    seen, todo = set(), list(succ[start])
    while todo:
        i = todo.pop()
        if i not in seen:
            seen.add(i)
            todo.extend(succ[i])
    return seen


def loop_of(succ, i):
    """the blocks on a cycle through block i (its strongly connected component), in layout order"""
    pred = [[] for _ in succ]
    for a, out in enumerate(succ):
        for b in out:
            pred[b].append(a)
    return sorted(reach(succ, i) & reach(pred, i))


def pick_loops(blocks, succ):
    """(consumer, producer): the loop around the block with the most v_pk_fma_f32, and the loop around the block with
    the most MFMAs outside it (stage B: v_mfma_f32_16x16x4_f32, or the 16x16x16 bf16 / f16 forms with LP != 0)"""
    st = max(range(len(blocks)), key=lambda i: blocks[i]["pk_fma"])
    cons = loop_of(succ, st) if blocks[st]["pk_fma"] else None
    rest = [i for i in range(len(blocks)) if not cons or i not in cons]
    sb = max(rest, key=lambda i: blocks[i]["counts"]["mfma"])
    prod = loop_of(succ, sb) if blocks[sb]["counts"]["mfma"] else None
    return cons or None, prod or None


def metadata(text, kernel):
    """the kernel's entry of the amdhsa.kernels metadata as a dict of its scalar fields"""
    i = text.index(".name:           " + kernel + "\n")
    a = text.rfind("\n  - .", 0, i)
    b = text.find("\n  - .", i)
    e = text.find("\namdhsa.target", i)
    b = e if b < 0 or (0 <= e < b) else b
    out = {}
    for m in re.finditer(r"^\s+(?:- )?\.(\w+):\s+(\S+)\s*$", text[a:b], re.M):
        out[m.group(1)] = int(m.group(2)) if re.fullmatch(r"-?\d+", m.group(2)) else m.group(2)
    return out


def report(text, kernel):
    blocks, succ = parse_kernel(text, kernel)
    cons, prod = pick_loops(blocks, succ)
    md = metadata(text, kernel)
    res = {"kernel": kernel,
           "vgprs": md.get("vgpr_count"), "agprs": md.get("agpr_count"), "sgprs": md.get("sgpr_count"),
           "vgpr_spills": md.get("vgpr_spill_count"), "sgpr_spills": md.get("sgpr_spill_count"),
           "scratch_bytes": md.get("private_segment_fixed_size"), "lds_bytes": md.get("group_segment_fixed_size"),
           "loops": {}}
    for role, l in (("consumer", cons), ("producer", prod)):
        if l is None:
            res["loops"][role] = None
            continue
        bl = []
        for i in l:
            blk = blocks[i]
            bl.append({"block": blk["name"], "instructions": blk["n"], **blk["counts"], "vm_waits": blk["vm_waits"],
                       "stencil": blk["pk_fma"] > 0})
        res["loops"][role] = {"blocks": bl, "totals": {k: sum(x[k] for x in bl) for k in KINDS}}
    return res


def show(res):
    print("%s" % res["kernel"])
    print("  VGPRs %s  AGPRs %s  SGPRs %s  spills v/s %s/%s  scratch %s B  LDS %s B" % (
        res["vgprs"], res["agprs"], res["sgprs"], res["vgpr_spills"], res["sgpr_spills"], res["scratch_bytes"], res["lds_bytes"]))
    for role in ("consumer", "producer"):
        lp = res["loops"][role]
        if lp is None:
            print("  %s loop: NOT FOUND" % role)
            continue
        print("  %s loop (%d blocks); a block of a branch is not executed in every sub-step" % (role, len(lp["blocks"])))
        print("    %-12s %5s %5s %6s %5s %4s %6s %5s  %s" % ("block", "instr", "mfma", "packed", "valu", "lds", "global", "smem", "s_waitcnt with vmcnt"))
        for b in lp["blocks"]:
            print("    %-12s %5d %5d %6d %5d %4d %6d %5d  %s%s" % (
                b["block"], b["instructions"], b["mfma"], b["packed"], b["valu"], b["lds"], b["global"], b["smem"],
                "; ".join(w.replace("s_waitcnt ", "") for w in b["vm_waits"]), "   <- stencil" if b["stencil"] else ""))
        t = lp["totals"]
        print("    %-12s %5s %5d %6d %5d %4d %6d %5d" % ("all blocks", "", t["mfma"], t["packed"], t["valu"], t["lds"], t["global"], t["smem"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--asm", help="read this assembly file instead of building one")
    ap.add_argument("--extra", type=int, default=0, help="EXTRA template argument (1: the heat map / probe forward)")
    ap.add_argument("--lp", type=int, default=0, help="LP template argument (0 fp32, 1 bf16, 2 fp16)")
    ap.add_argument("--flags", default="", help="extra compiler flags, e.g. -DOFX_HEAD_HOOKS=1")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    kernel = "_Z13k_head_streamILb%dELi%dEEv11HeadParams2" % (a.extra, a.lp)
    if a.asm:
        text = open(a.asm).read()
    else:
        if not find_hipcc():
            sys.exit("head_isa: no hipcc")
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "ofx_head.s")
            build_asm(path, a.flags.split())
            text = open(path).read()
    res = report(text, kernel)
    if a.json:
        print(json.dumps(res))
    else:
        show(res)


if __name__ == "__main__":
    main()
