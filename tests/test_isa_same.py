"""CPU: tools/isa_same.py on two made-up assembly directories -- a function that moved to another file with its block labels renumbered is the
same function; a changed instruction, a changed metadata value and a function on one side only are each named, with exit code 1."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unit(funcs):
    """funcs: [(name, block number, instruction, vgprs)] -> the text of a .s file"""
    body = "".join("\t.type\t%s,@function\n%s:                        ; @%s\n; %%bb.0:\n\ts_load_dword s0, s[0:1], 0x0\n.LBB%d_1:                    ; =>loop\n"
                   "\t%s\n\ts_cbranch_scc1 .LBB%d_1\n\ts_endpgm\n\t.section\t.rodata\n.Lfunc_end%d:\n\t.size\t%s, .Lfunc_end%d-%s\n"
                   % (n, n, n, b, ins, b, b, n, b, n) for n, b, ins, v in funcs)
    meta = "".join("  - .agpr_count:     0\n    .args:\n      - .offset:         0\n        .size:           8\n    .group_segment_fixed_size: 0\n"
                   "    .kernarg_segment_size: 8\n    .max_flat_workgroup_size: 64\n    .name:           %s\n    .private_segment_fixed_size: 0\n"
                   "    .sgpr_count:     8\n    .sgpr_spill_count: 0\n    .vgpr_count:     %d\n    .vgpr_spill_count: 0\n" % (n, v) for n, b, ins, v in funcs)
    return body + "\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + meta + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\n\t.end_amdgpu_metadata\n"


def same(tmp_path, tag, old, new):
    dirs = []
    for side, files in (("old", old), ("new", new)):
        d = tmp_path / (tag + "_" + side)
        d.mkdir()
        for f, funcs in files.items():
            (d / f).write_text(unit(funcs))
        dirs.append(str(d))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_same.py")] + dirs, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return p.returncode, p.stdout.decode()


def test_a_moved_function_is_the_same_and_every_change_is_named(tmp_path):
    a, b, c = ("k_a", 0, "s_add_u32 s1, s1, 1", 4), ("k_b", 1, "s_sub_u32 s1, s1, 1", 6), ("k_c", 2, "s_nop 0", 8)
    rc, out = same(tmp_path, "moved", {"one.s": [a, b, c]}, {"one.s": [a], "two.s": [("k_b", 0) + b[2:], ("k_c", 1) + c[2:]]})
    assert rc == 0 and "3 device function(s) in OLD, 3 in NEW" in out and "0 differ" in out, out
    rc, out = same(tmp_path, "instr", {"one.s": [a, b]}, {"one.s": [a, ("k_b", 1, "s_sub_u32 s1, s1, 2", 6)]})
    assert rc == 1 and "instructions differ" in out and "k_b" in out and "k_a" not in out, out
    rc, out = same(tmp_path, "meta", {"one.s": [a, b]}, {"one.s": [a, b[:3] + (7,)]})
    assert rc == 1 and "metadata differs" in out and "k_b" in out and "k_a" not in out, out
    rc, out = same(tmp_path, "gone", {"one.s": [a, b]}, {"one.s": [a], "two.s": [("k_c", 0) + c[2:]]})
    assert rc == 1 and "missing in NEW: k_b" in out and "missing in OLD: k_c" in out, out
