"""CPU: the compiler's resource lines of the five kernels of csrc/hip/k_markdup.hip from the cross-compiled code object: no LDS, no scratch, no
spilled registers, and few enough vector registers that a SIMD holds its eight waves -- the kernels wait on random 32-byte accesses, and
waves in flight are what hides them (DESIGN.md section 3 quotes the counts)."""
import os
import re
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_k_markdup_kernels_have_no_lds_no_scratch_and_at_most_64_vgprs(tmp_path):
    out = str(tmp_path / "k_markdup.s")
    p = subprocess.run([HIPCC, "-Wno-unused-command-line-argument", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + ROOT + "/include",
                        "-I" + ROOT + "/biscuit_amd/csrc/host", "-I" + ROOT + "/biscuit_amd/csrc/hip", "-S", "--cuda-device-only",
                        ROOT + "/biscuit_amd/csrc/hip/k_markdup.hip", "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    text = open(out).read()
    found = re.findall(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+_Z\d+(k_md_[a-z]+)(.*?)\.wavefront_size:\s+(\d+)", text, re.S)
    assert sorted(f[1] for f in found) == ["k_md_claim", "k_md_decide", "k_md_init", "k_md_publish", "k_md_rehash"], [f[1] for f in found]
    for lds, name, body, wave in found:
        vals = {k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1)) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
        assert int(lds) == 0 and vals["vgpr_spill_count"] == 0 and vals["sgpr_spill_count"] == 0 and vals["private_segment_fixed_size"] == 0, (name, lds, vals)
        assert int(wave) == 64 and vals["vgpr_count"] <= 64, (name, wave, vals)
    # the claim is a compare-and-swap and an atomic minimum in hardware (no emulation loop around another primitive)
    assert "global_atomic_cmpswap" in text and "global_atomic_umin" in text
