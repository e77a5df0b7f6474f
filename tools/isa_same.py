#!/usr/bin/env python3
"""Are two builds the same device code?  Usage: tools/isa_same.py OLD_ASM_DIR NEW_ASM_DIR   (directories of .s files, as tools/isa_check.sh
leaves under build/asm/).  Every device function is paired by its mangled name, whichever file holds it, and compared in (a) its instruction
lines -- comments and directives dropped, the labels .LBB<n>_<m> renamed .LBB_<m>, since <n> counts the functions ahead of it in its file --
and (b) its kernel metadata.  Names that differ or exist on one side only are printed; exit code 1 if there is one."""
import glob
import os
import re
import sys

META = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
        ".kernarg_segment_size", ".max_flat_workgroup_size")


def functions(d):
    """{mangled name: (instruction lines, {metadata key: value})} over every .s file of directory d"""
    code, meta = {}, {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        lines = open(path).read().split("\n")
        names = set(m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", l) for l in lines) if m)
        cur = None
        for l in lines:
            s = l.split(";")[0].strip()
            if s.endswith(":") and s[:-1] in names:
                cur = code.setdefault(s[:-1], [])
            elif s.startswith(".Lfunc_end"):
                cur = None
            elif cur is not None and s and (not s.startswith(".") or s.endswith(":")):
                cur.append(re.sub(r"\.L([A-Za-z]+)\d+_(\d+)", r".L\1_\2", s))
        # the metadata is a YAML list of kernels; within an entry the keys are sorted, so .name comes after some of the values
        for entry in re.split(r"\n  - (?=\.)", "\n".join(lines).partition("amdhsa.kernels:")[2].partition(".end_amdgpu_metadata")[0])[1:]:
            kv = dict(m.groups() for m in re.finditer(r"^\s*(\.\w+):\s*(\S+)\s*$", entry, re.M))
            if ".name" in kv:
                meta[kv[".name"]] = {k: kv.get(k) for k in META}
    return {n: (code[n], meta.get(n)) for n in code}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = functions(sys.argv[1]), functions(sys.argv[2])
    bad = 0
    for n in sorted(set(old) | set(new)):
        if n not in old or n not in new:
            print("%s: %s" % ("missing in NEW" if n in old else "missing in OLD", n))
        elif old[n][0] != new[n][0]:
            print("instructions differ (%d / %d lines): %s" % (len(old[n][0]), len(new[n][0]), n))
        elif old[n][1] != new[n][1]:
            print("metadata differs (%s / %s): %s" % (old[n][1], new[n][1], n))
        else:
            continue
        bad += 1
    print("%d device function(s) in OLD, %d in NEW, %d kernel(s) with metadata; %d differ or are missing" %
          (len(old), len(new), sum(1 for n in new if new[n][1]), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
