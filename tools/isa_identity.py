#!/usr/bin/env python3
"""Per-kernel instruction-stream identity of two gfx950 assembly listings (hipcc -save-temps: `*-hip-amdgcn-amd-amdhsa-gfx950.s`).

    python tools/isa_identity.py PARENT.s CHILD.s

Per kernel: the instruction lines between the kernel's label and its `.Lfunc_end` - comments, directives and the kernel descriptor dropped,
the function number in basic-block labels (`.LBB<n>_`) normalised - are counted and hashed (sha1, first 12 hex digits) in both listings.
Under a kernel: the descriptor fields (`.amdhsa_*`) that differ.  Kernels whose stream differs, and kernels only one side has, are listed with
their VGPR / SGPR / LDS / scratch figures.  Kernels are matched by their mangled symbol; a kernel that only one side has under its symbol is
matched by its DEMANGLED name where exactly one kernel of either side carries it (a template that gained a defaulted or empty parameter keeps
its demangled name and changes its symbol) and is marked "(by demangled name)".  Streams are compared as text: no instruction is interpreted.  Exit status 1 if any stream differs."""
import hashlib
import re
import shutil
import subprocess
import sys

FIGURES = (("VGPRs", "NumVgprs"), ("SGPRs", "TotalNumSgprs"), ("LDS", "LDSByteSize"), ("scratch", "ScratchSize"))


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    short = lambda s: re.sub(r"^void ", "", s.replace("(anonymous namespace)::", "")).split("(")[0]  # noqa: E731
    return {n: short(d) for n, d in zip(names, out)}


def kernels(path):
    """{name: dict(stream=[...], desc={field: value}, figures={...})} of every function that carries a kernel descriptor"""
    lines = open(path).read().split("\n")
    found, i = {}, 0
    while i < len(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):", lines[i])
        if not m or m.group(1).startswith(".L"):
            i += 1
            continue
        name, stream, desc, j = m.group(1), [], {}, i + 1
        while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
            text = lines[j].split(";")[0].strip()
            if text.startswith(".amdhsa_") and not text.startswith(".amdhsa_kernel"):
                field, _, value = text.partition(" ")
                desc[field] = value.strip()
            elif text and (not text.startswith(".") or text.startswith(".LBB")):
                stream.append(re.sub(r"\.LBB\d+_", ".LBB_", text))
            j += 1
        figures = {}
        while j < len(lines) and not re.match(r"^[A-Za-z_][\w$.]*:", lines[j]):
            for label, key in FIGURES:
                f = re.match(rf"^; {key}: (\d+)", lines[j])
                if f:
                    figures[label] = int(f.group(1))
            j += 1
        if desc:
            found[name] = dict(stream=[s for s in stream if not s.endswith(":")], labels=stream, desc=desc, figures=figures)
        i = j
    return found


def digest(k):
    return hashlib.sha1("\n".join(k["labels"]).encode()).hexdigest()[:12]


def figures(k):
    return " ".join(f"{label} {k['figures'].get(label, '?')}" for label, _ in FIGURES)


def main(parent_s, child_s):
    parent, child = kernels(parent_s), kernels(child_s)
    names = demangle(sorted(set(parent) | set(child)))
    print(f"{'kernel':<44}{'instr':>6}{'instr':>6}  {'sha1 parent':<13}{'sha1 child':<13}verdict")
    differ = 0
    pairs = {n: n for n in set(parent) & set(child)}  # parent symbol -> child symbol
    for s in {names[n] for n in parent if n not in child}:
        ps, cs = [n for n in parent if n not in child and names[n] == s], [n for n in child if n not in parent and names[n] == s]
        if len(ps) == 1 and len(cs) == 1:
            pairs[ps[0]] = cs[0]
    for n in sorted(pairs, key=names.get):
        p, c = parent[n], child[pairs[n]]
        same = digest(p) == digest(c)
        differ += not same
        print(f"{names[n]:<44}{len(p['stream']):>6}{len(c['stream']):>6}  {digest(p):<13}{digest(c):<13}{'identical' if same else 'DIFFERS'}" +
              ("" if pairs[n] == n else "  (by demangled name)"))
        fields = {f: (p["desc"].get(f), c["desc"].get(f)) for f in sorted(set(p["desc"]) | set(c["desc"])) if p["desc"].get(f) != c["desc"].get(f)}
        if fields:
            print(f"    descriptor fields that differ: {fields}")
        if not same:
            print(f"    parent: {figures(p)}\n    child:  {figures(c)}")
    for title, side, matched in (("only in the parent", parent, set(pairs)), ("new in the child", child, set(pairs.values()))):
        only = sorted(set(side) - matched, key=names.get)
        if only:
            print(f"{title}:")
        for n in only:
            print(f"   {names[n]} {len(side[n]['stream'])} instructions; {figures(side[n])}")
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
