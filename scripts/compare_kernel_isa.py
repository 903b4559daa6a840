#!/usr/bin/env python3
"""Compare the gfx950 kernels of two `make -C raytracing-in-a-weekend_amd/csrc asm` outputs.

    python scripts/compare_kernel_isa.py BEFORE_BUILD_DIR AFTER_BUILD_DIR [STEM [RESOURCE_FILE]]

Each directory holds what `make asm` writes to csrc/build/: rtw_kernels-hip-amdgcn-amd-amdhsa-gfx950.s and resource_usage.txt.
STEM names another translation unit of `make asm` (rtw_filter, rtw_query, rtw_occluded, rtw_refit, rtw_mesh_move): its
STEM-hip-amdgcn-amd-amdhsa-gfx950.s and RESOURCE_FILE, by default make asm's name for it (resource_usage_query.txt for rtw_query).
For every kernel of BEFORE, its body in AFTER (label to .Lfunc_end, with the .LBB<n>_ / .Lfunc_end<n> numbering normalised) and
its resource lines (VGPRs / SGPRs / scratch / occupancy / spills / LDS; source line numbers ignored) must be identical.  Assembler
comments are dropped before the comparison (their loop annotations carry the function's number too).  The
kernel descriptors (.amdhsa_kernel blocks) are compared as well and listed separately: they hold the size of the kernel-argument
block.  Kernels only in AFTER are listed with their resource lines.  Exit status 0 when every kernel of BEFORE is identical.
"""
import os
import re
import sys

STEM = "rtw_kernels"


def file_names(stem, res=None):
    """The assembly and the resource file of a translation unit as `make asm` names them."""
    return stem + "-hip-amdgcn-amd-amdhsa-gfx950.s", res or ("resource_usage.txt" if stem == STEM else "resource_usage_" + stem[len("rtw_"):] + ".txt")


def kernels(text):
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M)
    bodies, descs = {}, {}
    for k in names:
        m = re.search(r"^" + re.escape(k) + r":.*?^\.Lfunc_end\d+:", text, re.M | re.S)
        body = m.group(0) if m else ""
        body = re.sub(r"^\s*\.amdhsa_kernel .*?^\s*\.end_amdhsa_kernel", "", body, flags=re.M | re.S)   # the descriptor: compared on its own
        body = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", body)
        body = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", body)
        # assembler comments (loop annotations name blocks by the function's number) and the padding before them
        body = "\n".join(l for l in (re.sub(r"\s*;.*$", "", x).rstrip() for x in body.splitlines()) if l)
        bodies[k] = body
        d = re.search(r"^\s*\.amdhsa_kernel " + re.escape(k) + r"$.*?^\s*\.end_amdhsa_kernel", text, re.M | re.S)
        descs[k] = d.group(0) if d else ""
    return names, bodies, descs


def resources(text):
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: [^:]+:\d+:\d+: (.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        item = m.group(1).strip()
        if item.startswith("Function Name: "):
            cur = item[len("Function Name: "):]
            out[cur] = []
        elif cur is not None:
            out[cur].append(item)
    return out


def main():
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    asm, res = file_names(*(sys.argv[3:5] or [STEM]))
    ta, tb = (open(os.path.join(d, asm)).read() for d in (a_dir, b_dir))
    ra, rb = (resources(open(os.path.join(d, res)).read()) for d in (a_dir, b_dir))
    na, ba, da = kernels(ta)
    nb, bb, db = kernels(tb)
    same_body = same_res = same_desc = 0
    bad, desc_diffs = [], {}
    for k in na:
        if k not in bb:
            bad.append(f"MISSING in after: {k}")
            continue
        if ba[k] == bb[k]:
            same_body += 1
        else:
            bad.append(f"BODY differs: {k}")
        if ra.get(k) == rb.get(k):
            same_res += 1
        else:
            bad.append(f"RESOURCES differ: {k}: {ra.get(k)} -> {rb.get(k)}")
        if da[k] == db[k]:
            same_desc += 1
        else:
            diff = "; ".join(f"{x.strip()} -> {y.strip()}" for x, y in zip(da[k].splitlines(), db[k].splitlines()) if x != y)
            desc_diffs.setdefault(diff, []).append(k)
    print(f"kernels before: {len(na)}, after: {len(nb)}")
    print(f"bodies identical: {same_body}/{len(na)}; resource lines identical: {same_res}/{len(na)}; descriptors identical: {same_desc}/{len(na)}")
    for diff, ks in desc_diffs.items():
        print(f"descriptors of {len(ks)} kernels differ in: {diff}")
    for line in bad:
        print(line)
    new = [k for k in nb if k not in ba]
    for k in new:
        r = {x.split(":")[0]: x.split(":", 1)[1].strip() for x in rb.get(k, [])}
        print(f"new: {k}: VGPRs {r.get('VGPRs')}, SGPRs {r.get('TotalSGPRs')}, scratch {r.get('ScratchSize [bytes/lane]')} B/lane, "
              f"occupancy {r.get('Occupancy [waves/SIMD]')} waves/SIMD, VGPR spills {r.get('VGPRs Spill')}, SGPR spills {r.get('SGPRs Spill')}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
