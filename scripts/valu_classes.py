#!/usr/bin/env python3
"""Count a kernel's VALU instructions by issue class from the assembly `make -C raytracing-in-a-weekend_amd/csrc asm` writes.

    python scripts/valu_classes.py ASM_FILE [KERNEL_SUBSTRING] [--blocks] [--dump OUT.s]

Classes as measured by scripts/ubench/valu_mix.hip (profiles/r06_ubench_valu_mix.txt):
  fast   ~2.5 cycles per wave-instruction: fp32 mul / add / sub / fma, v_mov, two-operand integer add / sub / shift / and / or / xor
  slow   ~4.3: min / max (also the three-operand ones), compares, v_cndmask, conversions, integer multiplies, three-operand
         integer forms (v_bfe, v_lshl_add, v_add3, v_and_or, v_mad_u64_u32 ...), v_perm, v_alignbit, packed and mixed fma, lane reads
  trans  ~8: v_rcp, v_rsq, v_sqrt, v_exp, v_log, v_sin, v_cos
The default kernel is the bench build, render_bvh<false, 1, 1, false>.  --blocks lists the counts per basic block (label), in
program order, with the block's non-VALU instruction counts: the table of DESIGN.md 4.2 is made from it by naming the blocks.
--dump writes the kernel's body alone."""
import re
import sys

FAST = re.compile(r"^v_(mul_f32|add_f32|sub_f32|subrev_f32|fma_f32|fmac_f32|mac_f32|mad_f32|mov_b32|mov_b64|add_u32|sub_u32|subrev_u32|add_co_u32|"
                  r"sub_co_u32|subrev_co_u32|addc_co_u32|subb_co_u32|lshlrev_b32|lshrrev_b32|ashrrev_i32|and_b32|or_b32|xor_b32|not_b32|"
                  r"mul_legacy_f32|accvgpr_\w+|nop)(_e32|_e64|_dpp|_sdwa)?$")
TRANS = re.compile(r"^v_(rcp|rsq|sqrt|exp|log|sin|cos)_")


def classify(op):
    if not op.startswith("v_"):
        return None
    if TRANS.match(op):
        return "trans"
    if FAST.match(op):
        return "fast"
    return "slow"


def kernel_body(text, sub):
    names = [k for k in re.findall(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M) if sub in k]
    assert len(names) == 1, names
    m = re.search(r"^" + re.escape(names[0]) + r":.*?^\.Lfunc_end\d+:", text, re.M | re.S)
    return names[0], m.group(0)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    blocks = "--blocks" in sys.argv
    dump = sys.argv[sys.argv.index("--dump") + 1] if "--dump" in sys.argv else None
    if dump:
        args.remove(dump)
    sub = args[1] if len(args) > 1 else "render_bvhILb0ELi1ELi1ELb0EE"
    name, body = kernel_body(open(args[0]).read(), sub)
    if dump:
        open(dump, "w").write(body)
    tot = {"fast": 0, "slow": 0, "trans": 0, "salu": 0, "lds": 0, "vmem": 0, "smem": 0}
    per, order, cur = {}, [], "entry"
    for line in body.splitlines():
        s = re.sub(r"\s*;.*$", "", line).strip()
        if not s or s.startswith("."):
            m = re.match(r"^(\.LBB\d+_\d+):", s)
            if m:
                cur = m.group(1)
            continue
        if s.endswith(":"):
            continue
        op = s.split()[0]
        c = classify(op)
        if c is None:
            c = "salu" if op.startswith("s_") and not op.startswith(("s_load", "s_buffer_load", "s_waitcnt", "s_nop", "s_branch", "s_cbranch")) else \
                "smem" if op.startswith(("s_load", "s_buffer_load")) else "lds" if op.startswith("ds_") else \
                "vmem" if op.startswith(("global_", "flat_", "buffer_", "scratch_")) else None
        if c is None:
            continue
        tot[c] += 1
        if cur not in per:
            per[cur] = dict.fromkeys(tot, 0)
            order.append(cur)
        per[cur][c] += 1
    print(name)
    print("static: VALU %d = fast %d + slow %d + trans %d;  SALU %d, LDS %d, VMEM %d, SMEM %d" %
          (tot["fast"] + tot["slow"] + tot["trans"], tot["fast"], tot["slow"], tot["trans"], tot["salu"], tot["lds"], tot["vmem"], tot["smem"]))
    if blocks:
        for b in order:
            p = per[b]
            print("%-12s fast %3d slow %3d trans %2d | salu %3d lds %2d vmem %2d smem %2d" %
                  (b, p["fast"], p["slow"], p["trans"], p["salu"], p["lds"], p["vmem"], p["smem"]))


if __name__ == "__main__":
    main()
