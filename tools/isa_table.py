#!/usr/bin/env python3
"""Compare the pivot-update kernels of two builds of the csrc/*.hip kernel files, kernel by kernel.

    hipcc -O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 --cuda-device-only -S lpx_kernels.hip -o X.s
    python tools/isa_table.py PARENT.s BRANCH.s > profiles/rNN_tile_isa.md
    python tools/isa_table.py --parent A.s [B.s ...] --branch C.s [D.s ...] > profiles/rNN_tile_isa.md
    python tools/isa_table.py --diff PARENT.s BRANCH.s > profiles/rNN_tile_isa_diffs.txt

Each side is the device assembly of one or several files (one .s per .hip file); a kernel is found by name, whichever file
holds it.  --all: every kernel of the assemblies instead of the pivot-update kernels of the KERNELS pattern.
--diff: instead of the table, a unified diff of the two instruction streams (register numbers and labels blanked) of every
kernel whose streams are not the same text.  "The same text" leaves out the function number of .LBB<f>_<n> labels, which
counts the functions in front of the kernel in its file: a kernel that changed file or place keeps its text.

Per kernel: registers, scratch, LDS and occupancy from the code-object metadata, a histogram of the mnemonics that matter to a
streaming FP64 kernel (loads and stores split by `nt`), and whether the two instruction streams are the same text, the same
up to register numbers and labels, or different; a kernel that only one side has gets one row of its own figures.  Exit status 1 when a figure that admits no exception moved (VGPRs, scratch,
LDS, occupancy, FP64 counts -- v_fma_f64 among them -- and load and store counts per policy against the first file, or any
v_fma_f64 in a kernel without a division: with one, only the equal count says that the tile got none).
"""
import difflib
import re
import subprocess
import sys
from collections import Counter

KERNELS = re.compile(r"lpx::(lpx_update(_s|_m|_mb|_mb_s|_mb_m|_b|_mb_b)?|lpx_pivot_select|lpx_group_fused(_c)?)\(|"
                     r"lpx::lpx_pivot_fused(_c)?<\d+>\(")
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
COLS = ("ld_x4 nt", "ld_x4", "st_x4 nt", "st_x4", "flat", "v_mul_f64", "v_add_f64", "v_fma_f64", "v_div", "s_waitcnt", "branch")
STRICT = ("ld_x4 nt", "ld_x4", "st_x4 nt", "st_x4", "flat", "v_mul_f64", "v_add_f64", "v_fma_f64", "v_div")


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def classify(line):
    op = line.split()[0]
    nt = " nt" in line
    if op == "global_load_dwordx4":
        return "ld_x4 nt" if nt else "ld_x4"
    if op == "global_store_dwordx4":
        return "st_x4 nt" if nt else "st_x4"
    if op.startswith("flat_load") or op.startswith("flat_store"):
        return "flat"
    if op in ("v_mul_f64", "v_add_f64", "v_fma_f64", "s_waitcnt"):
        return op
    if op.startswith("v_div_"):
        return "v_div"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    return None


def normalise(line):
    line = re.sub(r"\b([vsa])\[\d+:\d+\]", r"\1[]", line)
    line = re.sub(r"\b([vsa])\d+\b", r"\1", line)
    return re.sub(r"\.LBB\d+_\d+", ".L", line)


def parse_all(paths, every):
    out = {}
    for path in paths:
        one = parse(path, every)
        dup = set(out) & set(one)
        if dup:
            sys.exit("kernel in two files of one side: " + ", ".join(sorted(dup)))
        out.update(one)
    return out


def parse(path, every=False):
    text = open(path).read().split("\n")
    meta, rec = {}, None
    for ln in text[text.index("amdhsa.kernels:"):]:     # the metadata at the end of the file: one "  - " record per kernel
        m = re.match(r"  (- |  )(\.[a-z_]+):\s*(\S+)\s*$", ln)
        if not m:
            continue
        if m.group(1) == "- ":
            rec = {}
        if m.group(2) == ".name":
            meta[m.group(3)] = rec
        elif m.group(2) in META:
            rec[m.group(2)] = int(m.group(3))
    names = demangle(sorted(meta))
    out = {}
    for mangled, rec in meta.items():
        nice = names[mangled]
        if not every and not KERNELS.search(nice):
            continue
        start = next(i for i, ln in enumerate(text) if ln.startswith(mangled + ":"))
        body, occ = [], None
        for i in range(start + 1, len(text)):
            s = text[i].split(";")[0].strip()
            if text[i].startswith(".Lfunc_end"):
                for j in range(i, min(i + 40, len(text))):
                    m = re.match(r";\s*Occupancy:\s*(\d+)", text[j].strip())
                    if m:
                        occ = int(m.group(1))
                        break
                break
            if s and not s.startswith(".") and not s.endswith(":"):
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))      # the function number: the kernel's place in its file
        short = re.sub(r"^lpx::", "", nice.split("(")[0])
        out[short] = {"meta": rec, "occ": occ, "body": body, "hist": Counter(filter(None, map(classify, body)))}
    return out


def order(name):
    m = re.match(r"(.*)<(\d+)>$", name)
    return (1, m.group(1), int(m.group(2))) if m else (0, name, 0)


def main():
    sides, cur = {"pos": [], "--parent": [], "--branch": []}, "pos"
    for a in sys.argv[1:]:
        if a in ("--parent", "--branch"):
            cur = a
        elif a not in ("--diff", "--all"):
            sides[cur].append(a)
    if len(sides["pos"]) == 2 and not sides["--parent"] and not sides["--branch"]:
        sides["--parent"], sides["--branch"] = sides["pos"][:1], sides["pos"][1:]
    elif sides["pos"] or not sides["--parent"] or not sides["--branch"]:
        sys.exit(__doc__)
    every = "--all" in sys.argv[1:]
    A, B = parse_all(sides["--parent"], every), parse_all(sides["--branch"], every)
    if "--diff" in sys.argv[1:]:
        for k in sorted(set(A) & set(B), key=order):
            a, b = [normalise(x) for x in A[k]["body"]], [normalise(x) for x in B[k]["body"]]
            if A[k]["body"] != B[k]["body"]:
                print("\n".join(difflib.unified_diff(a, b, k + " (first file)", k + " (second file)", lineterm="", n=2)))
        return 0
    bad = []
    if sorted(A) != sorted(B):
        bad.append("kernel sets differ: " + ", ".join(sorted(set(A) ^ set(B))))
    print("| kernel | side | VGPR | AGPR | SGPR | scratch | LDS | occ | " + " | ".join(COLS) + " | lines | stream |")
    print("|---|---|" + "---|" * (7 + len(COLS) + 1))
    for k in sorted(set(A) & set(B), key=order):
        a, b = A[k], B[k]
        if a["body"] == b["body"]:
            same = "identical text"
        elif [normalise(x) for x in a["body"]] == [normalise(x) for x in b["body"]]:
            same = "identical up to registers and labels"
        elif Counter(normalise(x) for x in a["body"]) == Counter(normalise(x) for x in b["body"]):
            same = "same instructions, order differs"
        else:
            d = Counter(normalise(x) for x in a["body"])
            d.subtract(Counter(normalise(x) for x in b["body"]))
            same = "differs (%d instructions)" % sum(abs(v) for v in d.values())
        for side, r in (("parent", a), ("branch", b)):
            mt = r["meta"]
            row = [k, side] + [str(mt.get(f, 0)) for f in META] + [str(r["occ"])] + [str(r["hist"][c]) for c in COLS]
            print("| " + " | ".join(row) + " | %d | %s |" % (len(r["body"]), same if side == "branch" else ""))
        for f in (".vgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size"):
            if a["meta"].get(f, 0) != b["meta"].get(f, 0):
                bad.append("%s: %s %d -> %d" % (k, f, a["meta"].get(f, 0), b["meta"].get(f, 0)))
        if a["occ"] != b["occ"]:
            bad.append("%s: occupancy %s -> %s" % (k, a["occ"], b["occ"]))
        for c in STRICT:
            if a["hist"][c] != b["hist"][c]:
                bad.append("%s: %s %d -> %d" % (k, c, a["hist"][c], b["hist"][c]))
        if b["hist"]["v_fma_f64"] and not b["hist"]["v_div"]:      # a division's expansion is the one place an FMA belongs
            bad.append("%s: v_fma_f64 present" % k)
    for k in sorted(set(A) ^ set(B), key=order):                   # a kernel only one side has: its own figures, nothing to compare
        side, r = ("parent", A[k]) if k in A else ("branch", B[k])
        row = [k, side] + [str(r["meta"].get(f, 0)) for f in META] + [str(r["occ"])] + [str(r["hist"][c]) for c in COLS]
        print("| " + " | ".join(row) + " | %d | %s only |" % (len(r["body"]), side))
    print()
    print("strict figures (VGPR, AGPR, scratch, LDS, occupancy, loads and stores per policy, FP64 counts, no FMA beside a division): " +
          ("all equal" if not bad else "MOVED"))
    for x in bad:
        print("- " + x)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
