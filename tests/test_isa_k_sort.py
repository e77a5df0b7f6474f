"""CPU: the compiler's resource lines of the six kernels of csrc/hip/k_sort.hip from the cross-compiled code object: wave64, no scratch, no
spilled registers, the LDS DESIGN.md section 3 states for each kernel, and few enough vector registers (64) in the kernels of the tiled passes
that a SIMD holds its eight waves -- they stream keys through HBM, and waves in flight are what hides that.  k_sort_small is one workgroup, a
wave per SIMD, whatever it takes: its bound (128) only keeps it from growing unnoticed.  Resource lines only."""
import os
import re
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TILE = 2048
# bytes of LDS: the wave rows of digit counts are 4 waves x 256 digits x 4 bytes; k_sort_small adds two buffers of TILE keys (8 bytes) and TILE
# payloads (4 bytes), the four wave totals of its scan and the OR word
LDS = {"k_sort_bits": 8, "k_sort_hist": 256 * 4, "k_sort_scan1": 16, "k_sort_scan2": 16, "k_sort_scatter": 4 * 256 * 4,
       "k_sort_small": 2 * TILE * 8 + 2 * TILE * 4 + 4 * 256 * 4 + 16 + 8}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_k_sort_kernels_are_wave64_without_scratch_or_spills_with_the_stated_lds(tmp_path):
    hdr = open(ROOT + "/include/bsx.h").read()
    assert int(re.search(r"#define BSX_SORT_TILE (\d+)", hdr).group(1)) == TILE
    out = str(tmp_path / "k_sort.s")
    p = subprocess.run([HIPCC, "-Wno-unused-command-line-argument", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + ROOT + "/include",
                        "-I" + ROOT + "/biscuit_amd/csrc/host", "-I" + ROOT + "/biscuit_amd/csrc/hip", "-S", "--cuda-device-only",
                        ROOT + "/biscuit_amd/csrc/hip/k_sort.hip", "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    text = open(out).read()
    found = re.findall(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+_Z\d+(k_sort_[a-z0-9]+)(.*?)\.wavefront_size:\s+(\d+)", text, re.S)
    assert sorted(f[1] for f in found) == sorted(LDS), [f[1] for f in found]
    for lds, name, body, wave in found:
        vals = {k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1)) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
        print(name, "lds", lds, vals)
        assert vals["vgpr_spill_count"] == 0 and vals["sgpr_spill_count"] == 0 and vals["private_segment_fixed_size"] == 0, (name, vals)
        assert int(wave) == 64 and vals["vgpr_count"] <= (128 if name == "k_sort_small" else 64), (name, wave, vals)
        assert int(lds) == LDS[name], (name, lds, LDS[name])
