"""CPU: the compiler's resource lines of k_qc (csrc/hip/k_qc.hip) from the cross-compiled code object: no scratch (no private segment, no
spilled vector registers) and less than 16 KB of LDS per workgroup -- the histograms of a block and its four waves' staged tiles -- so that
four workgroups fit a compute unit."""
import os
import re
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_k_qc_has_no_scratch_and_under_16k_of_lds(tmp_path):
    out = str(tmp_path / "k_qc.s")
    p = subprocess.run([HIPCC, "-Wno-unused-command-line-argument", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + ROOT + "/include",
                        "-I" + ROOT + "/biscuit_amd/csrc/host", "-I" + ROOT + "/biscuit_amd/csrc/hip", "-S", "--cuda-device-only",
                        ROOT + "/biscuit_amd/csrc/hip/k_qc.hip", "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    text = open(out).read()
    found = re.findall(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(_Z4k_qc\S*)(.*?)\.wavefront_size:\s+(\d+)", text, re.S)
    assert len(found) == 1, [f[1] for f in found]
    lds, name, body, wave = found[0]
    vals = {k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1)) for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    assert vals["vgpr_spill_count"] == 0 and vals["private_segment_fixed_size"] == 0, vals
    assert 2432 * 4 <= int(lds) < 16384, lds       # at least the block's 2 432 counters
    assert int(wave) == 64 and vals["vgpr_count"] <= 128, (wave, vals)
    assert "scratch_" not in text
