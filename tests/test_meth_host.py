"""CPU: the host side of the base-averaged conversion table (csrc/host/meth.c: the beta in thousandths against printf, the host statement of the
counting rule and of the table pass, the state of a backend without the device seam, the writer) in a stand-alone program,
tests/meth_host_main.c, built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_milli_rule_tables_state_and_writer_under_sanitizers(tmp_path):
    exe = str(tmp_path / "meth_host")
    out = tmp_path / "out"
    out.mkdir()
    src = ["tests/meth_host_main.c", "biscuit_amd/csrc/host/meth.c"]
    c = subprocess.run(["gcc", "-g", "-O1", "-std=gnu11", "-Wall", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-Iinclude", "-Ibiscuit_amd/csrc/host"] + src + ["-o", exe, "-lm", "-lpthread"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert c.returncode == 0, c.stdout.decode()[-3000:]
    p = subprocess.run([exe, str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and p.stdout == b"ok\n", (p.returncode, p.stderr.decode()[-3000:])
