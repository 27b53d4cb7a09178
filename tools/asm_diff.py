#!/usr/bin/env python3
"""Device assembly of every translation unit of csrc/ at a parent commit against the working tree, kernel by kernel.

usage: python tools/asm_diff.py <parent-ref> [file.hip ...] [-j JOBS] [--keep DIR]        (no files: all of SRCS)

Both trees are compiled with FLAGS of csrc/Makefile plus `--cuda-device-only -S` (the parent's sources come from
`git archive`, into a temporary directory).  Compared is what the assembler would see: comment lines, `.file` / `.loc` /
`.ident` / `.section` lines and the per-build `__hip_cuid_*` symbol are dropped; kernel metadata (`.amdhsa_*`, the
`amdhsa.kernels` block) stays.  Prints one line per kernel (or other symbol) that differs, `identical` lines per file
otherwise; exit status 1 on any difference.  A refactor of device code that claims "same code" is checked with this.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "taichi_3d_gaussian_splatting_amd/csrc"
DROP = re.compile(r"^\s*(;|//|\.file\b|\.loc\b|\.ident\b|\.section\b)|__hip_cuid_")


def makefile_vars(csrc):
    text = open(os.path.join(csrc, "Makefile")).read()
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}
    expand = lambda s: re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), s)
    return expand(var["HIPCC"]), expand(var["FLAGS"]).split(), var["SRCS"].split()


def compile_asm(hipcc, flags, csrc, src, out):
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s in %s failed:\n%s" % (" ".join(cmd), csrc, r.stdout))
    return out


def chunks(path):
    """filtered lines of an assembly file, keyed by the symbol they belong to ('' = file scope)"""
    out = {"": []}
    cur = ""
    meta = None                                   # lines of the current entry of amdhsa.kernels
    for line in open(path):
        line = line.rstrip()
        if not line or DROP.search(line):
            continue
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not line.startswith(".L"):
            cur = m.group(1)
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = m.group(1) + " (descriptor)"
        if re.match(r"^\s+- \.", line):           # a new entry of the metadata's kernel list
            if meta:
                out.setdefault(meta[0] + " (metadata)", []).extend(meta[1])
            meta = ["", []]
        if meta is not None:
            m = re.match(r"^\s+\.name:\s+(\S+)", line)
            if m:
                meta[0] = m.group(1)
            if line.startswith("amdhsa.target") or line.startswith("..."):
                out.setdefault(meta[0] + " (metadata)", []).extend(meta[1])
                meta = None
            else:
                meta[1].append(line)
                continue
        m = re.match(r"^\s*\.set\s+(\S+)\.\w+,", line)       # resource symbols of a kernel, emitted behind its body
        out.setdefault(m.group(1) if m else cur, []).append(line)
        if re.match(r"^\s*\.end_amdhsa_kernel", line) or re.match(r"^\.Lfunc_end", line):
            cur = ""
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("files", nargs="*")
    ap.add_argument("-j", "--jobs", type=int, default=min(9, os.cpu_count() or 1))
    ap.add_argument("--keep", help="directory that keeps the two sets of .s files")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        work = a.keep or tmp
        for side in ("parent_src", "parent", "new"):
            os.makedirs(os.path.join(work, side), exist_ok=True)
        archive = subprocess.run(["git", "-C", ROOT, "archive", a.parent, CSRC, "include"], check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", os.path.join(work, "parent_src")], input=archive, check=True)
        trees = {"parent": os.path.join(work, "parent_src", CSRC), "new": os.path.join(ROOT, CSRC)}
        srcs = a.files or makefile_vars(trees["new"])[2]
        jobs = {}
        with concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
            for side, csrc in trees.items():
                side_hipcc, side_flags, _ = makefile_vars(csrc)
                for src in srcs:
                    out = os.path.join(work, side, src.replace(".hip", ".s"))
                    jobs[side, src] = pool.submit(compile_asm, side_hipcc, side_flags, csrc, src, out)
            asm = {k: f.result() for k, f in jobs.items()}
        differ = 0
        for src in srcs:
            p, n = chunks(asm["parent", src]), chunks(asm["new", src])
            bad = [k for k in sorted(set(p) | set(n)) if p.get(k) != n.get(k)]
            for k in bad:
                pl, nl = p.get(k), n.get(k)
                what = "only in parent" if nl is None else "only in new" if pl is None else \
                    "%d -> %d lines, %d differ" % (len(pl), len(nl), sum(x != y for x, y in zip(pl, nl)) + abs(len(pl) - len(nl)))
                print("%s: DIFFERS %s: %s" % (src, k or "(file scope)", what))
            if not bad:
                print("%s: identical (%d symbols)" % (src, len(p)))
            differ += len(bad)
        return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
