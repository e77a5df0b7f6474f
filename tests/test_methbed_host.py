"""CPU: the host side of --meth-bed (csrc/host/meth.c: the host statement of the site rule with its windows, the state of a backend without the
device seam, the line formatter, the contig order and the writer) in a stand-alone program, tests/methbed_host_main.c, built with
AddressSanitizer and UndefinedBehaviorSanitizer and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sites_windows_lines_order_and_writer_under_sanitizers(tmp_path):
    exe = str(tmp_path / "methbed_host")
    out = tmp_path / "out"
    out.mkdir()
    src = ["tests/methbed_host_main.c", "biscuit_amd/csrc/host/meth.c"]
    c = subprocess.run(["gcc", "-g", "-O1", "-std=gnu11", "-Wall", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-Iinclude", "-Ibiscuit_amd/csrc/host"] + src + ["-o", exe, "-lm", "-lpthread"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert c.returncode == 0, c.stdout.decode()[-3000:]
    p = subprocess.run([exe, str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and p.stdout == b"ok\n", (p.returncode, p.stderr.decode()[-3000:])
