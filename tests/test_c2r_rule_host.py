"""CPU: the rules of mem_chain2region that the host's state machine and the region and extension kernels share (csrc/host/c2r_rule.h: a seed's
span, the window clamp, the containment and disagreement tests, a side's job, the band retry, local against to-the-end) in a stand-alone program,
tests/c2r_rule_host_main.c, over a table of designed edge cases with hand-worked values; built with AddressSanitizer and
UndefinedBehaviorSanitizer and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "c2r_rule_host")
    c = subprocess.run(["gcc", "-g", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-Ibiscuit_amd/csrc/host", "tests/c2r_rule_host_main.c", "-o", exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert c.returncode == 0 and c.stdout == b"", c.stdout.decode()[-3000:]
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and p.stdout == b"ok\n", (p.returncode, p.stderr.decode()[-3000:])
