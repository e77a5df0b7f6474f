"""CPU: the host side of --sort (csrc/host/sortout.c: keys from SAM lines, the host's stable merge sort, the temporary file, the merge through
buffers of 1, 7 and 4 096 bytes, an empty chunk, a record longer than the buffer, a failed write, the header) in a stand-alone program,
tests/sortout_host_main.c, built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keys_host_sort_temporary_file_and_merge_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sortout_host")
    src = ["tests/sortout_host_main.c", "biscuit_amd/csrc/host/sortout.c", "biscuit_amd/csrc/host/tune.c"]
    c = subprocess.run(["gcc", "-g", "-O1", "-std=gnu11", "-Wall", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-Iinclude", "-Ibiscuit_amd/csrc/host"] + src + ["-o", exe, "-lpthread"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert c.returncode == 0, c.stdout.decode()[-3000:]
    env = {k: v for k, v in os.environ.items() if k != "BSX_TUNE"}
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert p.returncode == 0 and p.stdout == b"ok\n", (p.returncode, p.stderr.decode()[-3000:])
