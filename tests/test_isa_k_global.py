"""CPU: the compiler's resource lines of k_global (csrc/hip/k_global.hip).  The counting of conversions by context is a second form of the
kernel (template parameter CTX); the plain form must stay the code it was: same vector registers, no spills, no scratch -- the values below
were recorded from the build of the commit before the form was added.  The new form must not spill either."""
import os
import re
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# NC -> .vgpr_count of k_global<NC> before the change (.vgpr_spill_count and .private_segment_fixed_size were 0 for all three)
RECORDED = {4: 134, 16: 150, 32: 212}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_plain_k_global_keeps_its_registers_and_the_ctx_form_does_not_spill(tmp_path):
    out = str(tmp_path / "k_global.s")
    p = subprocess.run([HIPCC, "-Wno-unused-command-line-argument", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + ROOT + "/include",
                        "-I" + ROOT + "/biscuit_amd/csrc/host", "-I" + ROOT + "/biscuit_amd/csrc/hip", "-S", "--cuda-device-only",
                        ROOT + "/biscuit_amd/csrc/hip/k_global.hip", "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    text = open(out).read()
    found = {}
    for m in re.finditer(r"\.name:\s+(_Z8k_globalILi(\d+)ELb([01])EE\S*)(.*?)\.wavefront_size", text, re.S):
        body = m.group(4)
        vals = {k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1)) for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
        found[(int(m.group(2)), int(m.group(3)))] = vals
    assert sorted(found) == [(nc, c) for nc in (4, 16, 32) for c in (0, 1)], sorted(found)
    for nc, vg in RECORDED.items():
        assert found[(nc, 0)] == {"vgpr_count": vg, "vgpr_spill_count": 0, "private_segment_fixed_size": 0}, (nc, found[(nc, 0)])
        assert found[(nc, 1)]["vgpr_spill_count"] == 0 and found[(nc, 1)]["private_segment_fixed_size"] == 0, (nc, found[(nc, 1)])
