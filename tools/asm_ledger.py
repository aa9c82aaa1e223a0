#!/usr/bin/env python3
"""Static instruction counts per basic block of one kernel in a gfx950 assembly file (hipcc -S
--cuda-device-only): VALU, SALU, LDS, branches and the block's successors, plus the kernel's
.vgpr_count / scratch / LDS size. The ledger of k_enc_parse (profiles/r08/enc_valu/ledger.md)
was made with it. Usage: python tools/asm_ledger.py FILE.s 'k_enc_parseILj2ELj0E' [-v]"""
import re
import sys


def main():
    path, key = sys.argv[1], sys.argv[2]
    verbose = "-v" in sys.argv
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(key) + r"\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    name = lines[start].split(":")[0]
    blocks, cur = [], {"label": "entry", "valu": 0, "salu": 0, "lds": 0, "vmem": 0, "br": [], "ops": []}
    for l in lines[start + 1:end]:
        t = l.strip()
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            blocks.append(cur)
            cur = {"label": m.group(1), "valu": 0, "salu": 0, "lds": 0, "vmem": 0, "br": [], "ops": []}
            continue
        if not t or t.startswith(";") or t.startswith("."):
            continue
        op = t.split()[0]
        cur["ops"].append(op)
        if op.startswith("v_"):
            cur["valu"] += 1
        elif op.startswith("ds_"):
            cur["lds"] += 1
        elif op.startswith(("global_", "flat_", "buffer_", "scratch_")):
            cur["vmem"] += 1
        elif op.startswith("s_"):
            cur["salu"] += 1
            if op.startswith(("s_cbranch", "s_branch")):
                cur["br"].append(t.split()[-1])
    blocks.append(cur)
    tot = {k: sum(b[k] for b in blocks) for k in ("valu", "salu", "lds", "vmem")}
    print(f"{name}\n{len(blocks)} blocks, static VALU {tot['valu']} SALU {tot['salu']} LDS {tot['lds']} VMEM {tot['vmem']}")
    for l in lines[end:]:
        if name in l and re.search(r"\.(num_vgpr|private_seg_size|num_agpr), ", l):
            print(" ", l.split(name)[-1].strip())
    for i in range(end, len(lines)):
        if lines[i].strip() == f".amdhsa_kernel {name}":
            for l in lines[i:i + 12]:
                if "group_segment" in l or "private_segment" in l:
                    print(" ", l.strip())
            break
    print("label valu salu lds vmem -> successors")
    for b in blocks:
        print(f"{b['label']:>12} {b['valu']:4d} {b['salu']:4d} {b['lds']:3d} {b['vmem']:3d} -> {' '.join(b['br'])}")
        if verbose:
            hist = {}
            for o in b["ops"]:
                if o.startswith("v_"):
                    hist[o] = hist.get(o, 0) + 1
            print("             " + ", ".join(f"{k} {v}" for k, v in sorted(hist.items(), key=lambda kv: -kv[1])))


if __name__ == "__main__":
    main()
