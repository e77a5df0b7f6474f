"""CPU: the host side of --bam (csrc/host/bam.c with csrc/host/bam_rec.h, the record rule the device compiles too: the header part, the name
table and its search, the records, every refusal, the host's deflate and framing, and the writer with its pieces, carried tail, refusals and
failing sink) in a stand-alone program, tests/bam_host_main.c, built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_records_refusals_name_table_and_writer_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bam_host")
    src = ["tests/bam_host_main.c", "biscuit_amd/csrc/host/bam.c", "biscuit_amd/csrc/host/tune.c"]
    c = subprocess.run(["gcc", "-g", "-O1", "-std=gnu11", "-Wall", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-Iinclude", "-Ibiscuit_amd/csrc/host"] + src + ["-o", exe, "-lz", "-lm", "-lpthread"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert c.returncode == 0, c.stdout.decode()[-3000:]
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and p.stdout == b"ok\n", (p.returncode, p.stderr.decode()[-3000:])
