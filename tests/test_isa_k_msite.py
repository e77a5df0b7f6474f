"""CPU: the compiler's resource lines of both kernels of csrc/hip/k_msite.hip from the cross-compiled code object: no scratch (no private segment,
no spilled vector or scalar registers), the LDS each one declares -- two sets of four wave totals, 32 bytes, as the file's head documents --
wave size 64, and the vector registers the finished kernels have.  Metadata lines only."""
import os
import re
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# kernel (mangled prefix) -> (LDS bytes, vector registers)
WANT = {"_Z13k_msite_count": (32, 32), "_Z12k_msite_emit": (32, 44)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_k_msite_kernels_have_no_scratch_and_the_pinned_lds_and_registers(tmp_path):
    out = str(tmp_path / "k_msite.s")
    p = subprocess.run([HIPCC, "-Wno-unused-command-line-argument", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + ROOT + "/include",
                        "-I" + ROOT + "/biscuit_amd/csrc/host", "-I" + ROOT + "/biscuit_amd/csrc/hip", "-S", "--cuda-device-only",
                        ROOT + "/biscuit_amd/csrc/hip/k_msite.hip", "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    text = open(out).read()
    found = re.findall(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(_Z\d+k_msite\S*)(.*?)\.wavefront_size:\s+(\d+)", text, re.S)
    seen = {}
    for lds, name, body, wave in found:
        key = [k for k in WANT if name.startswith(k)]
        assert len(key) == 1, name
        vals = {k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1)) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
        assert vals["vgpr_spill_count"] == 0 and vals["sgpr_spill_count"] == 0 and vals["private_segment_fixed_size"] == 0, (name, vals)
        assert int(wave) == 64 and int(lds) == WANT[key[0]][0] and vals["vgpr_count"] == WANT[key[0]][1], (name, lds, wave, vals)
        seen[key[0]] = name
    assert sorted(seen) == sorted(WANT), sorted(seen)
