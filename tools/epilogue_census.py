#!/usr/bin/env python3
"""Static census of the tile epilogue in a gfx950 assembly listing (hipcc -S --cuda-device-only) of one of the
LDS-staged GEMM sources.  Per kernel: VGPR / AGPR / SGPR counts and scratch size from the code-object metadata, and, for
the text after the last MFMA: instructions, vector-memory loads and stores, branches, and the lengths of the store runs --
maximal sequences of stores with no load, no `s_waitcnt vmcnt`, no branch and no label between two of them.

    python tools/epilogue_census.py conv_gemm_x6.s [name-filter]
"""
import collections
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def census(path, name_filter=""):
    lines = open(path).read().splitlines()
    meta, cur = {}, None
    for ln in lines:
        s = ln.strip()
        m = re.match(r"(?:- )?\.(name|vgpr_count|agpr_count|sgpr_count|private_segment_fixed_size):\s*(\S+)", s)
        if not m:
            continue
        if s.startswith("- ."):
            cur = {}                    # a new kernel's map starts at its first key
        if cur is None:
            continue
        cur[m.group(1)] = m.group(2)
        if m.group(1) == "name":
            meta[m.group(2)] = cur
    bodies, name, body = {}, None, []
    for ln in lines:
        m = re.match(r"^(_Z\w+):", ln)
        if m and m.group(1) in meta:
            name, body = m.group(1), []
            continue
        if name is not None:
            if ln.startswith(".Lfunc_end"):
                bodies[name] = body
                name = None
            else:
                body.append(ln.split(";")[0].strip())
    pretty = demangle(list(bodies))
    rows = []
    for name, body in bodies.items():
        if name_filter not in pretty[name]:
            continue
        ins = [b for b in body if b and not b.startswith(".") or re.match(r"\.LBB\w+:", b or "")]
        last = max((i for i, b in enumerate(ins) if b.startswith("v_mfma")), default=-1)
        tail = ins[last + 1:]
        n_ins = n_ld = n_st = n_br = 0
        runs, run = [], 0
        for b in tail:
            op = b.split()[0]
            is_label = op.endswith(":")
            is_st = re.match(r"(global|buffer|flat)_store", op) is not None
            is_ld = re.match(r"(global|buffer|flat)_load", op) is not None
            is_br = op.startswith("s_cbranch") or op == "s_branch"
            is_wait = op == "s_waitcnt" and "vmcnt" in b
            if not is_label:
                n_ins += 1
            n_ld += is_ld
            n_st += is_st
            n_br += is_br
            if is_st:
                run += 1
            elif run and (is_ld or is_br or is_wait or is_label):
                runs.append(run)
                run = 0
        if run:
            runs.append(run)
        md = meta[name]
        rows.append((pretty[name], md.get("vgpr_count"), md.get("agpr_count", "0"), md.get("sgpr_count"),
                     md.get("private_segment_fixed_size"), n_ins, n_ld, n_st, n_br,
                     " ".join(f"{k}x{v}" for k, v in sorted(collections.Counter(runs).items(), reverse=True))))
    return rows


if __name__ == "__main__":
    print("| kernel | VGPR | AGPR | SGPR | scratch | instr after last MFMA | loads | stores | branches | store runs (length x count) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in sorted(census(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "")):
        print("| `" + re.sub(r"^void ", "", r[0]).replace("(CGParams)", "") + "` | " + " | ".join(str(x) for x in r[1:]) + " |")
