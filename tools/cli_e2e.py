#!/usr/bin/env python3
"""End-to-end run of the command line (FASTQ parse -> align -> SAM text written), the figure SURVEY 8(d) asks for
next to the in-memory bench: python tools/cli_e2e.py [--genome-mbp 128] [--chunks 6]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--genome-mbp", type=float, default=128)
ap.add_argument("--chunks", default="6", help="chunks of reads in the FASTQ files; two numbers a,b: two runs, and the steady-state rate from their difference")
ap.add_argument("--profile", type=int, default=0, help="0: the clean synthetic genome, 1: the hg38-like one (csrc/host/sim.c)")
ap.add_argument("--json", action="store_true", help="one JSON line (bench.py's cli_end_to_end sub-record)")
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--out", default=None, help="where the SAM goes (default: a file in the work directory; /dev/null isolates the aligner from the write)")
ap.add_argument("--align-args", default="", help="further options for biscuit_align, space separated (e.g. --bsconv)")
ap.add_argument("--wrap", default="", help="a command to run biscuit_align under, space separated, ending in -- where it wants one (e.g. a kernel trace of the run)")
a = ap.parse_args()
from biscuit_amd import _lib as B
from biscuit_amd.api import Index, Device
L = B.lib()
n_bases = int(a.genome_mbp * 1e6)
work = "/tmp/bsx_bench_%d_p%d" % (n_bases, a.profile)
base = work + "/g"
t_build = None
if not os.path.exists(base + ".dau.sa"):
    os.makedirs(work, exist_ok=True)
    tb = time.time()
    if n_bases > 1_000_000_000:   # past the host builder's 32-bit suffix sorter: both indices on the device, then the seven files
        g = Index.synthetic(n_bases, seed=2024, n_contigs=24, profile=a.profile)
        dev = Device(0)
        dev.build_index(g, fill_host=True)
        g.save(base)
        dev.close(); g.close()
    else:
        B.check(L.bsx_sim_genome((work + "/g.fa").encode(), C.c_int64(n_bases), C.c_uint64(2024), 8, C.c_double(0.05)), "sim_genome")
        B.check(L.bsx_index_build((work + "/g.fa").encode(), base.encode()), "index_build")
    t_build = round(time.time() - tb, 1)
idx = Index(base)
L.bsx_sim_pairs.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_void_p)]
L.bsx_sim_write_fastq.argtypes = [C.c_void_p, C.c_int64, C.c_char_p, C.c_char_p, C.c_int]
L.bsx_sim_free_reads.argtypes = [C.c_void_p, C.c_int64]
pairs = 10000000 * a.threads // 300
fq1, fq2 = work + "/e2e_1.fq", work + "/e2e_2.fq"
runs = []
env = dict(os.environ)
env.setdefault("BSX_HOST_THREADS", str(a.threads))
written = 0
import threading
for n_chunks in sorted(int(x) for x in a.chunks.split(",")):
    for k in range(written, n_chunks):   # the longer run's files continue the shorter one's
        p = C.c_void_p()
        B.check(L.bsx_sim_pairs(idx.h, pairs, 150, 4000 + k, 200, 500, 0.005, 0.0, C.byref(p)), "sim_pairs")
        B.check(L.bsx_sim_write_fastq(p, 2 * pairs, fq1.encode(), fq2.encode(), 1 if k else 0), "write_fastq")
        L.bsx_sim_free_reads(p, 2 * pairs)
    written = n_chunks
    outp = a.out or (work + "/e2e.sam")
    done_at, err_lines = [], []
    t0 = time.time()
    with open(outp, "wb") as sam:
        pr = subprocess.Popen(a.wrap.split() + [os.path.join(ROOT, "biscuit_amd", "biscuit_align")] + a.align_args.split() + ["-@", str(a.threads), base, fq1, fq2],
                              stdout=sam, stderr=subprocess.PIPE, env=env)

        def watch():   # when each chunk's SAM is complete: the command line says so on stderr ([M::bsx_process_seqs] Processed ...)
            for line in pr.stderr:
                err_lines.append(line)
                if b"Processed" in line:
                    done_at.append(time.time() - t0)
        th = threading.Thread(target=watch)
        th.start()
        rc = pr.wait()
        th.join()
    dt = time.time() - t0
    assert rc == 0, b"".join(err_lines)[-2000:].decode(errors="replace")
    if os.environ.get("E2E_STDERR"):
        open(os.environ["E2E_STDERR"], "wb").write(b"".join(err_lines))
    r = {"chunks": n_chunks, "reads": 2 * pairs * n_chunks, "seconds": round(dt, 2), "reads_per_s_whole_process": round(2 * pairs * n_chunks / dt, 1),
         "chunk_done_at_s": [round(x, 2) for x in done_at]}
    if len(done_at) >= 3:   # chunks complete at the stream's rate once the pipeline is full: first completion to last
        r["steady_state_s_per_chunk"] = round((done_at[-1] - done_at[0]) / (len(done_at) - 1), 3)
        r["steady_state_reads_per_s"] = round(2 * pairs / max(1e-9, r["steady_state_s_per_chunk"]), 1)
        r["start_up_and_fill_s"] = round(done_at[0], 2)
    runs.append(r)
idx.close()
res = {"metric": "reads/s through the command line: FASTQ text in -> SAM text out (biscuit_align -@ %d <index files> r1.fq r2.fq > %s)" % (a.threads, a.out or "file"),
       "align_args": a.align_args, "runs": runs, "genome_mbp": a.genome_mbp, "genome_profile": "hg38-like" if a.profile else "clean", "genome_and_index_files_s": t_build,
       "includes": "index files -> host -> HBM, dense SA sample and table of k-mer intervals rebuilt on the device, FASTQ parse, alignment, SAM text written",
       "steady_state_is": "the time from the first chunk's SAM being complete to the last one's, per chunk (the start-up -- index load and upload, pipeline fill -- is reported beside it)"}
best = runs[-1]
res["value"], res["unit"] = best.get("steady_state_reads_per_s", best["reads_per_s_whole_process"]), "reads/s"
print(json.dumps(res) if a.json else res)
