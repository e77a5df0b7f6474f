"""CPU: the compiler's resource lines of the kernels of csrc/hip/k_bam.hip and csrc/hip/k_bgzf.hip from the cross-compiled code objects: no
scratch (no private segment, no spilled vector or scalar registers), wave size 64, and the LDS each one declares -- k_bam_count and k_bam_starts
two sets of four wave totals (32 bytes), k_bam_scan sixteen wave totals and the carry (68), k_bam_refused one 64-bit word, the line kernel none,
k_bgzf_deflate its whole BgzfLds (the block, the match table, the histograms and code tables: 138 848 bytes, one workgroup per compute unit), the
compaction none.  Metadata lines only."""
import os
import re
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# file -> kernel (mangled prefix) -> LDS bytes
WANT = {"k_bam": {"_Z11k_bam_count": 32, "_Z10k_bam_scan": 68, "_Z12k_bam_starts": 32, "_Z11k_bam_lines": 0, "_Z13k_bam_refused": 8},
        "k_bgzf": {"_Z14k_bgzf_deflate": 138848, "_Z14k_bgzf_compact": 0}}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("stem", sorted(WANT))
def test_kernels_have_no_scratch_no_spills_and_the_pinned_lds(tmp_path, stem):
    out = str(tmp_path / (stem + ".s"))
    p = subprocess.run([HIPCC, "-Wno-unused-command-line-argument", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + ROOT + "/include",
                        "-I" + ROOT + "/biscuit_amd/csrc/host", "-I" + ROOT + "/biscuit_amd/csrc/hip", "-S", "--cuda-device-only",
                        ROOT + "/biscuit_amd/csrc/hip/%s.hip" % stem, "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    text = open(out).read()
    found = re.findall(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(_Z\d+k_b\S*)(.*?)\.wavefront_size:\s+(\d+)", text, re.S)
    seen = {}
    for lds, name, body, wave in found:
        key = [k for k in WANT[stem] if name.startswith(k)]
        assert len(key) == 1, name
        vals = {k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1)) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
        assert vals["vgpr_spill_count"] == 0 and vals["sgpr_spill_count"] == 0 and vals["private_segment_fixed_size"] == 0, (name, vals)
        assert int(wave) == 64 and int(lds) == WANT[stem][key[0]] and vals["vgpr_count"] <= 128, (name, lds, wave, vals)
        assert int(lds) <= 160 * 1024
        seen[key[0]] = name
    assert sorted(seen) == sorted(WANT[stem]), sorted(seen)
