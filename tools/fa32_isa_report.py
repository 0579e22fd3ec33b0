"""Tile-loop instruction counts of the 32x32 flash kernels, from built extensions:

    python tools/fa32_isa_report.py PARENT/_C*.so BRANCH/_C*.so

The method of profiles/fa32_helpers_isa.txt: the gfx950 code object is
unbundled from each .so (.hip_fatbin -> clang-offload-bundler), disassembled
with llvm-objdump and split per kernel symbol; register, LDS and scratch
figures come from the code object's amdhsa metadata (llvm-readelf --notes).

Per kernel the tile loop is the span of the longest backward branch.  It is cut
into basic blocks at every branch and branch target, and each block is counted
by instruction class ("vmcnt" = the s_waitcnt that carry a vmcnt field).  A
block with 16 or more v_cmp and no MFMA is a causal-mask block: "unmasked
path" sums the loop without those.  Blocks are listed in address order, which
is the compiler's layout and not always execution order.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

KERNELS = ("fa_fwd_bf16", "fa2_dq_bf16", "fa2_dk_bf16", "fa2_dv_bf16", "fa2_dvdk_bf16")
CLASSES = ("VALU", "v_exp", "v_cmp", "v_cndmask", "v_permlane32_swap", "ds_read", "ds_write",
           "MFMA", "s_waitcnt", "vmcnt", "s_barrier", "vmem")


def _tool(name):
    found = shutil.which(name)
    if found:
        return found
    return os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name)


def code_object(so, tmp, tag):
    fat = os.path.join(tmp, tag + ".fatbin")
    co = os.path.join(tmp, tag + ".co")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, so,
                    os.path.join(tmp, tag + ".unused")], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--unbundle",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co], check=True)
    return co


def metadata(co):
    text = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True,
                          capture_output=True, text=True).stdout
    out, cur = {}, {}
    for line in text.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(\S+)", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2)
        if key == "agpr_count":  # first key of a kernel's record
            cur = {}
        cur[key] = val
        if key == "name":
            out[val] = cur
    return out


def disassemble(co):
    """{symbol: [(address, mnemonic, operands)]}"""
    text = subprocess.run([_tool("llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True,
                          capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if m and cur is not None:
            cur.append((int(m.group(3), 16), m.group(1), m.group(2)))
    return out


def classify(mn, ops=""):
    got = []
    if mn.startswith("s_waitcnt") and "vmcnt" in ops:
        got.append("vmcnt")
    if mn.startswith("v_mfma"):
        got.append("MFMA")
    elif mn.startswith("v_"):
        got.append("VALU")
    for c in ("v_exp", "v_cmp", "v_cndmask", "v_permlane32_swap", "ds_read", "ds_write",
              "s_waitcnt", "s_barrier"):
        if mn.startswith(c):
            got.append(c)
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        got.append("vmem")
    return got


def branch_target(ins, nxt):
    """Address a branch jumps to: objdump prints the signed word offset."""
    _, mn, ops = ins
    if not (mn.startswith("s_cbranch") or mn == "s_branch"):
        return None
    m = re.match(r"(-?\d+)", ops)
    if not m:
        return None
    off = int(m.group(1))
    if off >= 32768:
        off -= 65536
    return nxt + 4 * off


def tile_loop(insns):
    addrs = [a for a, _, _ in insns]
    best = None
    for i, ins in enumerate(insns):
        nxt = addrs[i + 1] if i + 1 < len(insns) else ins[0] + 4
        t = branch_target(ins, nxt)
        if t is not None and t <= ins[0] and (best is None or ins[0] - t > best[1] - best[0]):
            best = (t, ins[0])
    if best is None:
        return [], []
    body = [x for x in insns if best[0] <= x[0] <= best[1]]
    cuts = {best[0]}
    for i, ins in enumerate(body):
        nxt = body[i + 1][0] if i + 1 < len(body) else ins[0] + 4
        t = branch_target(ins, nxt)
        if t is not None:
            cuts.add(nxt)
            if best[0] <= t <= best[1]:
                cuts.add(t)
    blocks, cur = [], []
    for ins in body:
        if ins[0] in cuts and cur:
            blocks.append(cur)
            cur = []
        cur.append(ins)
    if cur:
        blocks.append(cur)
    return body, blocks


def count(insns):
    c = dict.fromkeys(CLASSES, 0)
    for _, mn, ops in insns:
        for k in classify(mn, ops):
            c[k] += 1
    return c


def fmt(c):
    return " ".join(f"{c[k]:>5}" for k in CLASSES)


def report(label, so, tmp):
    co = code_object(so, tmp, label)
    meta, dis = metadata(co), disassemble(co)
    print(f"== {label}: {os.path.basename(so)}")
    for k in KERNELS:
        m = meta.get(k, {})
        print(f"{k}: vgpr={m.get('vgpr_count')} agpr={m.get('agpr_count')} sgpr={m.get('sgpr_count')} "
              f"lds={m.get('group_segment_fixed_size')} scratch={m.get('private_segment_fixed_size')} "
              f"vgpr_spill={m.get('vgpr_spill_count')} sgpr_spill={m.get('sgpr_spill_count')} "
              f"instructions={len(dis.get(k, []))}")
        body, blocks = tile_loop(dis.get(k, []))
        print(f"  {'tile loop':<22}" + " ".join(f"{c[:5]:>5}" for c in CLASSES))
        total = count(body)
        unmasked = dict(total)
        for i, b in enumerate(blocks):
            c = count(b)
            mask = c["v_cmp"] >= 16 and c["MFMA"] == 0
            if mask:
                for kk in CLASSES:
                    unmasked[kk] -= c[kk]
            print(f"  block {i:<2} {len(b):>4} insns{'  mask' if mask else '      '} " + fmt(c))
        print(f"  {'all blocks':<22}" + fmt(total))
        print(f"  {'unmasked path':<22}" + fmt(unmasked))
    print()


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        for i, so in enumerate(sys.argv[1:]):
            report(("parent", "branch")[i] if len(sys.argv) == 3 else f"so{i}", so, tmp)


if __name__ == "__main__":
    main()
