"""CPU: `--bam` through the command line over the CPU restatement of the kernels (oracle_align: the backend without the two seams, i.e. the
host's own statement of both stages in bam.c -- bam_rec.h's records, zlib's deflate) on command lines of tests/e2e_cases.py: every member's
header fields, CRC and ISIZE (zlib inflates each as one gzip member), the EOF block, the joined payload against tests/bam_model.py's encoding of
the SAM the same command line writes without the option; two chunk sizes and small pieces give the same payload; --sort and --markdup --sort;
the emit hook's refusal with ranks; the refusals, each with status 1 and no output.  The -m gpu counterpart (tests/test_gpu_bam.py) puts
k_bam.hip and k_bgzf.hip on the other side."""
import os
import pytest
import bam_cases as BC
import bam_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "oracle", "oracle_align")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bam"))
    BC.make_data(d)
    return d


@pytest.mark.parametrize("case", [c for c, _ in BC.CASES])
def test_payload_is_the_models_encoding_of_the_plain_sam(data, case):
    sam, bam = BC.run_pair(CPU, [], dict(BC.CASES)[case], data)
    payload, n_h = BC.check_bam(bam, sam, case)
    assert len(payload) > n_h or case == "none"


def test_chunk_size_and_piece_size_do_not_change_the_payload(data):
    args = dict(BC.CASES)["se150"]                                               # (single reads: the records do not depend on the chunks)
    sam, bam = BC.run_pair(CPU, [], args, data)
    want, n_h = BC.check_bam(bam, sam, "one chunk")
    assert len(want) - n_h > M.BGZF_BLOCK                                       # more than a block: a record straddles two
    sam2, bam2 = BC.run_pair(CPU, [], args, data, env={"BSX_CHUNK_SIZE": "20000"})
    assert sam2 == sam and BC.check_bam(bam2, sam2, "small chunks")[0] == want
    for piece in ("1", "1000", "65280", "70001"):                                # a line a piece; pieces that end inside blocks and block_size fields
        _, bam3 = BC.run_pair(CPU, [], args, data, bam_env={"BSX_TUNE": "bam_piece_bytes=" + piece})
        assert bam3 == bam, piece                                                 # the host's deflate is a function of the block: the same file


def test_with_sort_and_with_markdup_and_sort(data):
    args = dict(BC.CASES)["pe150_b0"]
    for opts in (["--sort"], ["--markdup", "--sort"], ["--bsconv", "--markdup"]):
        sam, bam = BC.run_pair(CPU, opts, args, data, env={"BSX_CHUNK_SIZE": "20000"})
        payload, n_h = BC.check_bam(bam, sam, " ".join(opts))
        text = M.split_payload(payload)[0]
        assert text.startswith(b"@HD\tVN:1.6\tSO:coordinate\n") == ("--sort" in opts)


def test_an_input_without_reads_is_a_header_and_the_eof_block(data):
    open(data + "/none.fq", "w").close()
    sam, bam = BC.run_pair(CPU, [], ["-@", "1", "g", "none.fq"], data)
    payload, n_h = BC.check_bam(bam, sam, "no reads")
    assert len(payload) == n_h


def _refused(args, d, env=None):
    p = BC.run_raw(CPU, args, d, env)
    assert p.returncode == 1 and p.stdout == b"", (args, p.returncode, len(p.stdout), p.stderr.decode()[-1000:])
    return p.stderr.decode()


def test_refusals(data):
    d = data
    seq = "ACGTTGCATGCCGATAGCTAGGATCGATCGGCTAGCTAGGCTAACGATCGATTAGC"
    # (the aligner writes no field a tag rule refuses -- a -C comment is joined to the read name, as the reference does -- so those refusals are
    # tested at the seam: tests/test_bam_model.py, tests/bam_host_main.c, tests/test_gpu_bam.py.  Here: what a command line can reach.)
    # a comment that makes the name too long
    with open(d + "/c.fq", "w") as f:
        f.write("@ok short\n%s\n+\n%s\n@%s %s\n%s\n+\n%s\n" % (seq, "I" * len(seq), "n" * 200, "c" * 54, seq, "I" * len(seq)))
    p = BC.run_raw(CPU, ["--bam", "g", "c.fq"], d)
    assert p.returncode == 0 and len(M.split_payload(M.bgzf_payload(p.stdout))[2]) == 2
    assert "record 1 cannot be written as BAM: a read name longer than 254 bytes" in _refused(["--bam", "-C", "g", "c.fq"], d)
    # a read name of 255 bytes (254 pass)
    with open(d + "/n.fq", "w") as f:
        f.write("@%s\n%s\n+\n%s\n@%s\n%s\n+\n%s\n" % ("n" * 254, seq, "I" * len(seq), "m" * 255, seq, "I" * len(seq)))
    assert "record 1 cannot be written as BAM: a read name longer than 254 bytes" in _refused(["--bam", "g", "n.fq"], d)
    # a header whose @SQ lines leave out the contig the reads align to
    with open(d + "/sq.txt", "w") as f:
        f.write("@SQ\tSN:elsewhere\tLN:1000\n")
    err = _refused(["--bam", "-@", "4", "-H", "sq.txt", "g", "b1.fq"], d)
    assert "cannot be written as BAM: an RNAME or RNEXT without an @SQ line" in err
    # with --sort the first refused record of the sorted stream
    assert "record 1 cannot be written as BAM: a read name" in _refused(["--bam", "--sort", "-C", "g", "c.fq"], d)
    # options
    assert "--bam encodes SAM records: it cannot be combined with -F" in _refused(["--bam", "-F", "g", "b1.fq"], d)
    err = _refused(["--bam", "g", "b1.fq"], d, env={"RANK": "0", "WORLD_SIZE": "2", "LOCAL_RANK": "0", "LOCAL_WORLD_SIZE": "2", "BSX_GATHER_ID": d + "/never"})
    assert "--bam cuts the records of the whole output into blocks through one writer on one device: it cannot run with WORLD_SIZE > 1" in err
    assert not os.path.exists(d + "/never") and not os.path.exists(d + "/never.0")


def test_option_off_writes_what_it_wrote(data):
    args = dict(BC.CASES)["se150"]
    a = BC.run_raw(CPU, args, data).stdout
    b = BC.run_raw(CPU, args, data, env={"BSX_TUNE": "bam_piece_bytes=1"}).stdout
    assert a == b and a.startswith(b"@SQ")
