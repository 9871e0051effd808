#!/usr/bin/env python3
"""Compare the gfx950 assembly of two builds, device function by device function.

    make -C gpgradpy_amd/csrc EXTRA=--save-temps        (in two trees)
    tools/isa_diff.py OLD_DIR NEW_DIR [--allow NAME ...] [--allow-file FILE]

Both directories hold the *-hip-amdgcn-amd-amdhsa-gfx950.s files hipcc leaves behind with --save-temps.  Every file is split
into functions (the line "<mangled name>:" up to its .Lfunc_end label), trailing ';' comments are dropped, and the texts are
compared.  The ordinal of the function inside its file, which the assembler's local labels carry (.LBB12_3), is taken out
first: it changes when another function of the file appears or leaves.  Per function the tool prints identical / different /
missing / new and, for a kernel, the register counts and the scratch size of its metadata on both sides (--quiet leaves the
identical ones out, --show N adds the first lines of the textual diff).  The exit status is 1 when a function that is not on the allow list (mangled names, or substrings of them) is different,
missing or new, else 0.  Text is compared; nothing is searched for.
"""
import argparse
import difflib
import glob
import os
import re
import sys

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"
LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
LOCAL = re.compile(r"\.L(BB|JTI|CPI|tmp)\d+")
META = ("vgpr_count", "sgpr_count", "private_segment_fixed_size")


def split_functions(path):
    """({mangled name: normalised text}, {kernel name: {metadata key: int}}) of one assembly file"""
    funcs, meta = {}, {}
    name, body, kernel = None, [], None
    with open(path) as f:
        for raw in f:
            line = raw.split(";", 1)[0].rstrip()
            m = LABEL.match(line)
            if m:                                    # a global label opens a candidate; only a function reaches .Lfunc_end
                name, body = m.group(1), []
            elif line.startswith(".Lfunc_end"):
                if name is not None:
                    funcs[name] = "\n".join(body)
                name = None
            elif raw.startswith("    ."):            # metadata: "    .name: <kernel>" and the counts that follow it
                t = line.split()
                if len(t) == 2 and t[0] == ".name:":
                    kernel = t[1]
                    meta[kernel] = {}
                elif len(t) == 2 and kernel and t[0][1:-1] in META:
                    meta[kernel][t[0][1:-1]] = int(t[1])
            elif name is not None and line.strip():
                body.append(LOCAL.sub(lambda l: ".L" + l.group(1), line))
    return funcs, meta


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--allow", nargs="*", default=[], help="functions that may differ (mangled names or substrings)")
    ap.add_argument("--allow-file", help="file with one such name per line")
    ap.add_argument("--show", type=int, default=0, metavar="N", help="print the first N lines of the diff of every different function")
    ap.add_argument("--quiet", action="store_true", help="do not list the identical functions")
    a = ap.parse_args()
    allow = list(a.allow)
    if a.allow_file:
        with open(a.allow_file) as f:
            allow += [ln.strip() for ln in f if ln.strip()]

    units = sorted({os.path.basename(p) for d in (a.old, a.new) for p in glob.glob(os.path.join(d, "*" + SUFFIX))})
    if not units:
        print("no *%s files" % SUFFIX)
        return 2
    bad = 0
    for unit in units:
        sides = []
        for d in (a.old, a.new):
            p = os.path.join(d, unit)
            sides.append(split_functions(p) if os.path.exists(p) else ({}, {}))
        (fo, mo), (fn, mn) = sides
        count = {"identical": 0, "different": 0, "missing": 0, "new": 0}
        for name in sorted(set(fo) | set(fn)):
            state = "new" if name not in fo else "missing" if name not in fn else "identical" if fo[name] == fn[name] else "different"
            count[state] += 1
            regs = "  ".join("%s %s -> %s" % (k, mo.get(name, {}).get(k, "-"), mn.get(name, {}).get(k, "-")) for k in META)
            if state == "identical":
                if not a.quiet:
                    print("identical  %s\n           %s" % (name, regs))
                continue
            allowed = any(x in name for x in allow)
            bad += 0 if allowed else 1
            print("%-10s %s%s\n           %s" % (state, name, "  (allowed)" if allowed else "", regs))
            if state == "different" and a.show:
                delta = difflib.unified_diff(fo[name].split("\n"), fn[name].split("\n"), "old", "new", n=2, lineterm="")
                print("\n".join(list(delta)[: a.show]))
        print("== %s: %s" % (unit[: -len(SUFFIX)], ", ".join("%d %s" % (v, k) for k, v in count.items())))
    print("%d function(s) differ outside the allow list" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
