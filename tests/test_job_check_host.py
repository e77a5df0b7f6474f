"""CPU: the CIGAR walk that the output passes' batches check their jobs with (csrc/hip/job_check.h: range inside the pool, ops 0..4, the two
64-bit sums) in a stand-alone program, tests/job_check_host_main.c, built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cigar_walk_under_sanitizers(tmp_path):
    exe = str(tmp_path / "job_check_host")
    c = subprocess.run(["gcc", "-g", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-Ibiscuit_amd/csrc/hip", "tests/job_check_host_main.c", "-o", exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert c.returncode == 0 and c.stdout == b"", c.stdout.decode()[-3000:]
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and p.stdout == b"ok\n", (p.returncode, p.stderr.decode()[-3000:])
