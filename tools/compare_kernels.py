#!/usr/bin/env python3
"""Show that a change to the host side of csrc/ left every kernel as it was.

Each csrc/*.hip of two source trees is compiled to gfx950 device assembly with the flags of
katsdpsigproc_amd.build_native (FLAGS, PER_SOURCE_FLAGS of the tree this tool lies in) and cut
into functions, `.type <sym>,@function` to the matching `.size`. A whole-file diff would not
do: the order in which the compiler emits template instantiations depends on where the host
code names them, and local labels (.LBB<n>_<m>, .Lfunc_end<n>) carry the function's ordinal
in the file. So comments are dropped, that ordinal is taken out of the labels, and functions
are compared by symbol: their instruction streams, the `.amdhsa_` directives of a kernel's
descriptor and the `.set <sym>.<resource>` lines after it (registers, LDS, scratch).

Per source file the report names the symbols only in the old tree, only in the new tree,
and those whose instructions or descriptor differ. The exit status is 1 if there is any
difference other than an `--expect-removed SYMBOL` missing from the new tree (or if one of
those is still there), or if a file of the new tree yields no kernel at all and is not
named as `--host-only FILE.hip` (a translation unit without device code).

usage: tools/compare_kernels.py OLD_TREE NEW_TREE [--expect-removed SYMBOL]...
                                [--host-only FILE.hip]... [--only FILE.hip]...
                                [--jobs N] [--keep DIR]
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join("katsdpsigproc_amd", "csrc")

_TYPE = re.compile(r"^\.type\s+(\S+),@function$")
_SIZE = re.compile(r"^\.size\s+(\S+),")
_SET = re.compile(r"^\.set\s+(\S+)\.(\w+),\s*(.*)$")
# .LBB12_3 -> .LBB_3, .LJTI12_0 -> .LJTI_0, .Lfunc_end12 -> .Lfunc_end
_LOCAL = re.compile(r"\.L([A-Za-z]+)\d+_(\d+)")
_FUNC = re.compile(r"\.Lfunc_(begin|end)\d+")


def normalise(line):
    """One line of assembly without its comment and without the function's ordinal."""
    line = line.split(";", 1)[0].strip()
    line = _LOCAL.sub(r".L\1_\2", line)
    return _FUNC.sub(r".Lfunc_\1", line)


def parse(text):
    """{symbol: (instructions, descriptor)} of the functions in one file of assembly.

    Both are tuples of normalised lines; the descriptor (.amdhsa_ directives and .set
    resources) is empty for a device function that is no kernel and sets nothing.
    """
    code, desc = {}, {}
    current = None
    in_descriptor = False
    for raw in text.splitlines():
        line = normalise(raw)
        if not line:
            continue
        m = _SET.match(line)
        if m and m.group(1) in desc:
            desc[m.group(1)].append(f".set {m.group(2)} {m.group(3)}")
            continue
        if current is None:
            m = _TYPE.match(line)
            if m:
                current = m.group(1)
                code[current], desc[current] = [], []
            continue
        m = _SIZE.match(line)
        if m and m.group(1) == current:
            current = None
        elif line.startswith(".amdhsa_kernel"):
            in_descriptor = True
        elif line.startswith(".end_amdhsa_kernel"):
            in_descriptor = False
        elif in_descriptor:
            desc[current].append(line)
        else:
            code[current].append(line)
    return {sym: (tuple(code[sym]), tuple(desc[sym])) for sym in code}


def is_kernel(function):
    return any(line.startswith(".amdhsa_") for line in function[1])


def compare(old, new):
    """The differences between two parse() results, as four sorted lists of symbols."""
    both = old.keys() & new.keys()
    return {
        "only_old": sorted(old.keys() - new.keys()),
        "only_new": sorted(new.keys() - old.keys()),
        "code": sorted(s for s in both if old[s][0] != new[s][0]),
        "descriptor": sorted(s for s in both if old[s][1] != new[s][1]),
    }


def _flags():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from katsdpsigproc_amd import build_native

    return build_native._hipcc(), build_native.FLAGS, build_native.PER_SOURCE_FLAGS


def assemble(tree, name, out):
    hipcc, flags, per_source = _flags()
    cmd = [hipcc] + flags + per_source.get(name, []) + [
        "--cuda-device-only", "-S", os.path.join(tree, CSRC, name), "-o", out]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}\n{proc.stdout}\n{proc.stderr}")
    with open(out) as f:
        return parse(f.read())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--expect-removed", action="append", default=[], metavar="SYMBOL")
    ap.add_argument("--host-only", action="append", default=[], metavar="FILE.hip")
    ap.add_argument("--only", action="append", default=[], metavar="FILE.hip")
    ap.add_argument("--jobs", type=int, default=6)
    ap.add_argument("--keep", metavar="DIR", help="leave the assembly files in DIR")
    args = ap.parse_args()

    def sources(tree):
        return {os.path.basename(p) for p in glob.glob(os.path.join(tree, CSRC, "*.hip"))}

    names = sorted(sources(args.old_tree) | sources(args.new_tree))
    if args.only:
        names = [n for n in names if n in args.only]
    tmp = args.keep or tempfile.mkdtemp(prefix="compare_kernels_")
    jobs = []
    for side, tree in (("old", args.old_tree), ("new", args.new_tree)):
        os.makedirs(os.path.join(tmp, side), exist_ok=True)
        for name in names:
            if name in sources(tree):
                jobs.append((side, tree, name, os.path.join(tmp, side, name[:-4] + ".s")))
    with ThreadPoolExecutor(max_workers=max(1, args.jobs)) as pool:
        parsed = list(pool.map(lambda j: assemble(j[1], j[2], j[3]), jobs))
    result = {(j[0], j[2]): p for j, p in zip(jobs, parsed)}

    expected = set(args.expect_removed)
    seen_removed = set()
    bad = False
    total = kernels = 0
    for name in names:
        old, new = result.get(("old", name)), result.get(("new", name))
        if old is None or new is None:
            print(f"{name}: only in the {'new' if old is None else 'old'} tree")
            bad = True
            continue
        d = compare(old, new)
        n_kernels = sum(is_kernel(f) for f in new.values())
        total += len(new)
        kernels += n_kernels
        unexpected = [s for s in d["only_old"] if s not in expected]
        seen_removed.update(s for s in d["only_old"] if s in expected)
        same = len(new) - len(d["only_new"]) - len(set(d["code"]) | set(d["descriptor"]))
        print(f"{name}: {len(new)} functions ({n_kernels} kernels), {same} identical to the old "
              f"tree's, {len(d['only_old'])} removed ({len(unexpected)} unexpected), "
              f"{len(d['only_new'])} new, {len(d['code'])} with other instructions, "
              f"{len(d['descriptor'])} with another descriptor")
        for label, symbols in (("removed (expected)", sorted(set(d["only_old"]) & expected)),
                               ("REMOVED", unexpected), ("NEW", d["only_new"]),
                               ("INSTRUCTIONS DIFFER", d["code"]),
                               ("DESCRIPTOR DIFFERS", d["descriptor"])):
            for s in symbols:
                print(f"    {label}: {s}")
        no_kernels = n_kernels == 0 and name not in args.host_only
        if no_kernels:
            print("    NO KERNELS in this file")
        bad = bad or bool(unexpected or d["only_new"] or d["code"] or d["descriptor"]) or no_kernels
    for s in sorted(expected - seen_removed):
        print(f"expected to be removed but not removed (or never there): {s}")
        bad = True
    print(f"{len(names)} files, {total} functions ({kernels} kernels) in the new tree, "
          f"{len(seen_removed)} expected removals: {'DIFFERENCES' if bad else 'no kernel changed'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
