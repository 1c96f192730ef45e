"""Instruction census of a kernel's largest MFMA loop, from the assembly `hipcc -S` writes.  No GPU needed.

    python tools/isa_census.py audioeditingcode_amd/csrc/attention_x6.hip [--kernel attention_x6] [--arch gfx950]
    python tools/isa_census.py some_kernel.s

For every kernel (optionally only those whose name contains --kernel) it finds the loops (a conditional or unconditional
branch back to a label that was defined earlier in the same kernel), takes the one with the most MFMAs, and counts what
the matrix pipe has to share its issue slots with.  A loop with forward branches inside (a wave-uniform skip) is counted
whole, so the figures are an upper bound for a trip that takes the skip.  Prints one markdown table row per kernel:

    MFMA | trans (v_exp / v_log / v_rcp ...) | packed (v_pk_*) | other vector | all non-MFMA vector | per MFMA | LDS | memory | scalar
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")
LABEL = re.compile(r"^([.\w$]+):")
BRANCH = re.compile(r"^\s+s_c?branch\w*\s+([.\w$]+)")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)\b")


def kernels(lines):
    """(name, [lines]) for every kernel body of the file: from its label to its s_endpgm-terminated end."""
    names = {m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))}
    cur, body = None, []
    for ln in lines:
        m = LABEL.match(ln)
        if m and m.group(1) in names:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if ln.lstrip().startswith(".amdhsa_kernel") or ln.lstrip().startswith(".section"):
            yield cur, body
            cur = None
            continue
        body.append(ln)
    if cur is not None:
        yield cur, body


def classify(op):
    if op.startswith(("v_mfma", "v_smfma")):
        return "mfma"
    if op.startswith(TRANS):
        return "trans"
    if op.startswith("v_pk_"):
        return "packed"
    if op.startswith("v_"):
        return "vector"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "mem"
    if op.startswith("s_"):
        return "scalar"
    return None


def census(body, every=False):
    """Counts of the loop with the most MFMAs, plus a histogram of its vector opcodes (every: the list of all MFMA loops in
    program order, each with its scalar histogram as a third element)."""
    labels, best, loops = {}, None, []
    for n, ln in enumerate(body):
        m = LABEL.match(ln)
        if m:
            labels[m.group(1)] = n
            continue
        m = BRANCH.match(ln)
        if m and m.group(1) in labels:                                   # a back edge: the loop is body[label .. here]
            cnt, hist, shist = dict.fromkeys(("mfma", "trans", "packed", "vector", "lds", "mem", "scalar"), 0), {}, {}
            for l2 in body[labels[m.group(1)]:n + 1]:
                mi = INSN.match(l2)
                kind = classify(mi.group(1)) if mi else None
                if kind:
                    cnt[kind] += 1
                    if kind in ("trans", "packed", "vector"):
                        hist[mi.group(1)] = hist.get(mi.group(1), 0) + 1
                    if kind == "scalar":
                        shist[mi.group(1)] = shist.get(mi.group(1), 0) + 1
            if cnt["mfma"]:
                loops.append((cnt, hist, shist))
            if best is None or cnt["mfma"] > best[0]["mfma"]:
                best = (cnt, hist)
    return loops if every else best


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if tool is None:
        return {n: n for n in names}
    try:
        out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, (re.sub(r"^void |\(.*$", "", o) for o in out)))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("path", help="a .hip source (compiled with hipcc -S) or an assembly file")
    ap.add_argument("--kernel", default="", help="only kernels whose (demangled) name contains this")
    ap.add_argument("--arch", default=os.environ.get("AED_ARCH", "gfx950"))
    ap.add_argument("--top", type=int, default=0, help="also list the N most frequent vector opcodes of each loop")
    ap.add_argument("--all-loops", action="store_true",
                    help="one row per MFMA loop of a kernel, in program order (a kernel that picks one of several K loops per launch)")
    a = ap.parse_args()
    if a.path.endswith(".s"):
        text = open(a.path).read()
    else:
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "k.s")
            subprocess.check_call(["hipcc", "-S", "--cuda-device-only", f"--offload-arch={a.arch}", "-O3", "-std=c++17",
                                   a.path, "-o", out])
            text = open(out).read()
    found = list(kernels(text.split("\n")))
    names = demangle([n for n, _ in found])
    print("| kernel | MFMA | trans | packed | other vector | non-MFMA vector | per MFMA | LDS | memory | scalar |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for name, body in found:
        if a.kernel not in names[name] and a.kernel not in name:
            continue
        best = census(body)
        if best is None or best[0]["mfma"] == 0:
            print(f"| `{names[name]}` | no MFMA loop | | | | | | | | |")
            continue
        rows = [(names[name], best[0], best[1], None)]
        if a.all_loops:
            rows = [(f"{names[name]} loop {n}", *lp) for n, lp in enumerate(census(body, every=True))]
        for label, c, hist, shist in rows:
            nv = c["trans"] + c["packed"] + c["vector"]
            print(f"| `{label}` | {c['mfma']} | {c['trans']} | {c['packed']} | {c['vector']} | {nv} | {nv / c['mfma']:.1f} | "
                  f"{c['lds']} | {c['mem']} | {c['scalar']} |")
            if a.top:
                top = sorted(hist.items(), key=lambda kv: -kv[1])[:a.top]
                print("|  | " + ", ".join(f"{k} {v}" for k, v in top) + " | | | | | | | | |")
                if shist:
                    top = sorted(shist.items(), key=lambda kv: -kv[1])[:a.top]
                    print("|  | " + ", ".join(f"{k} {v}" for k, v in top) + " | | | | | | | | |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
