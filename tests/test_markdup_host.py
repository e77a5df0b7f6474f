"""CPU: the host side of duplicate marking (csrc/host/markdup.c: key construction, the host table with growth and salts, the tickets) in a
stand-alone program, tests/markdup_host_main.c, built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_table_keys_and_tickets_under_sanitizers(tmp_path):
    exe = str(tmp_path / "markdup_host")
    src = ["tests/markdup_host_main.c", "biscuit_amd/csrc/host/markdup.c", "biscuit_amd/csrc/host/tune.c"]
    c = subprocess.run(["gcc", "-g", "-O1", "-std=gnu11", "-Wall", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-Iinclude", "-Ibiscuit_amd/csrc/host"] + src + ["-o", exe, "-lpthread"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert c.returncode == 0, c.stdout.decode()[-3000:]
    env = {k: v for k, v in os.environ.items() if k != "BSX_TUNE"}
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert p.returncode == 0 and p.stdout == b"ok\n", (p.returncode, p.stderr.decode()[-3000:])
