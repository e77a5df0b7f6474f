"""CPU: tests/bam_model.py, the reference statement of --bam, on hand-worked records: the expected bytes of three records
written out by hand, every integer tag boundary, the bin of POS 0 and of alignments that end across the 2^14 .. 2^26 boundaries, odd and even
l_seq, SEQ and QUAL `*`, every CIGAR letter, the three kinds of RNEXT, a negative TLEN, decode(encode(line)) == line, every refusal, and the
block framing.  The same lines go through the library's host statement (csrc/host/bam_rec.h, the source the device compiles too), which must
give the model's bytes and the model's refusals."""
import struct
import zlib
import pytest
import bam_model as M

HDR = b"@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:300000000\n@SQ\tSN:chr2\tLN:5000\n@SQ\tSN:chr1\tLN:7\n@PG\tID:x\n"
IDS = M.ref_ids(M.header_refs(HDR))

R1 = b"r1\t99\tchr1\t100\t60\t5M\t=\t200\t105\tACGTN\tIIIII\tNM:i:0"
B1 = bytes.fromhex("33000000" "00000000" "63000000" "03" "3c" "4912" "0100" "6300" "05000000" "00000000" "c7000000" "69000000"
                   "723100" "50000000" "1248f0" "2828282828" "4e4d4300")
R2 = b"r2\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*"
B2 = bytes.fromhex("23000000" "ffffffff" "ffffffff" "03" "00" "4812" "0000" "0400" "00000000" "ffffffff" "ffffffff" "00000000" "723200")
R3 = b"r3\t147\tchr2\t1\t0\t2S3M\tchr1\t5\t-7\tACGTA\t*\tXA:A:x\tPA:f:0.500\tZZ:Z:hi\tXN:i:-129"
B3 = bytes.fromhex("49000000" "01000000" "00000000" "03" "00" "4912" "0200" "9300" "05000000" "00000000" "04000000" "f9ffffff"
                   "723300" "24000000" "30000000" "124810" "ffffffffff" "58414178" "5041660000003f" "5a5a5a686900" "584e737fff")


def lib_encode(text, hdr=HDR):
    """the host statement: (payload, bad record or -1, why)"""
    from biscuit_amd import api
    return api.bam_encode(None, hdr, text)


def both(line):
    """the model's record, checked against the host statement"""
    want = M.encode_record(line, IDS)
    got, bad, why = lib_encode(line + b"\n")
    assert (got, bad) == (want, -1), (line, got.hex(), want.hex(), bad, why)
    return want


def test_three_records_byte_for_byte():
    assert both(R1) == B1 and both(R2) == B2 and both(R3) == B3
    body, bad = M.encode_body(R1 + b"\n" + R2 + b"\n" + R3 + b"\n", IDS)
    assert bad is None and body == B1 + B2 + B3
    assert lib_encode(R1 + b"\n" + R2 + b"\n" + R3 + b"\n") == (B1 + B2 + B3, -1, 0)


def test_header_part():
    h = M.encode_header(HDR)
    want = b"BAM\1" + struct.pack("<i", len(HDR)) + HDR + struct.pack("<i", 3)
    want += struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 300000000) + struct.pack("<i", 5) + b"chr2\0" + struct.pack("<i", 5000) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 7)
    assert h == want
    assert IDS == {b"chr1": 0, b"chr2": 1}                                   # the first of two equal names
    from biscuit_amd import api, _lib
    assert api.bam_header(HDR) == want
    assert (_lib.BGZF_BLOCK, _lib.BAM_E_LINE, _lib.BAM_E_TAG, _lib.BAM_E_INT, _lib.BAM_E_NAME, _lib.BAM_E_CIGAR, _lib.BAM_E_REF, _lib.BAM_E_QUAL) == \
        (M.BGZF_BLOCK, M.E_LINE, M.E_TAG, M.E_INT, M.E_NAME, M.E_CIGAR, M.E_REF, M.E_QUAL)


@pytest.mark.parametrize("v,typ,fmt", [(-(1 << 31), "i", "<i"), (-32769, "i", "<i"), (-32768, "s", "<h"), (-129, "s", "<h"), (-128, "c", "<b"), (-1, "c", "<b"),
                                       (0, "C", "<B"), (255, "C", "<B"), (256, "S", "<H"), (65535, "S", "<H"), (65536, "I", "<I"), ((1 << 31) - 1, "I", "<I"),
                                       ((1 << 31), "I", "<I"), ((1 << 32) - 1, "I", "<I")])
def test_integer_tag_boundaries(v, typ, fmt):
    rec = both(R2 + b"\tXY:i:%d" % v)
    assert rec[4 + 35:] == b"XY" + typ.encode() + struct.pack(fmt, v)


def test_bins():
    def bin_of(line):
        return struct.unpack_from("<H", both(line), 4 + 10)[0]
    assert bin_of(b"r\t4\t*\t0\t0\t*\t*\t0\t0\tACG\t*") == 4680 == M.reg2bin(-1, 0)   # POS 0: beg = -1, L = 1, arithmetic shifts
    assert bin_of(b"r\t0\tchr1\t0\t0\t3M\t*\t0\t0\tACG\t*") == 0 == M.reg2bin(-1, 2)   # (a placed record there spans -1 .. 1: no bin below the root holds both)
    for k, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        e = 1 << k                                                               # an alignment [e - 2, e + 1) ends across 2^k
        inside = bin_of(b"r\t0\tchr1\t%d\t0\t2M\t*\t0\t0\tAC\t*" % (e - 2))       # [e - 3, e - 1): still inside the finer bin
        across = bin_of(b"r\t0\tchr1\t%d\t0\t3M\t*\t0\t0\tACG\t*" % (e - 1))
        assert inside == M.reg2bin(e - 3, e - 1) and across == M.reg2bin(e - 2, e + 1) and inside != across, (k, inside, across)
        assert inside >= first
    assert bin_of(b"r\t0\tchr1\t%d\t0\t3M\t*\t0\t0\tACG\t*" % ((1 << 26) - 1)) == 0   # across 2^26: the root bin
    # D, N, = and X count towards the end, I, S, H and P do not; 0x4 and CIGAR * give one position
    assert bin_of(b"r\t0\tchr1\t16384\t0\t1M1D1N1=1X5I5S\t*\t0\t0\tACGTACGTACGTA\t*") == M.reg2bin(16383, 16388)
    assert bin_of(b"r\t4\tchr1\t16384\t0\t10M\t*\t0\t0\tACGTACGTAC\t*") == M.reg2bin(16383, 16384)
    assert bin_of(b"r\t0\tchr1\t16384\t0\t*\t*\t0\t0\tACGTACGTAC\t*") == M.reg2bin(16383, 16384)
    assert bin_of(b"r\t0\tchr1\t16384\t0\t5I\t*\t0\t0\tACGTA\t*") == M.reg2bin(16383, 16384)


def test_seq_qual_cigar_rnext():
    odd = both(b"r\t0\tchr1\t1\t0\t3M\t*\t0\t0\tACG\t!~I")
    assert odd[4 + 32 + 2 + 4:] == bytes([0x12, 0x40, 0, 93, 40])                # the spare low nibble is 0
    even = both(b"r\t0\tchr1\t1\t0\t4M\t*\t0\t0\tTNac\t*")
    assert even[4 + 32 + 2 + 4:] == bytes([0x8f, 0xff, 255, 255, 255, 255])      # other letters give 15; QUAL * with a SEQ gives 0xff
    allseq = both(b"r\t0\tchr1\t1\t0\t*\t*\t0\t0\t=ACMGRSVTWYHKDBN\t*")
    assert allseq[4 + 32 + 2:4 + 32 + 2 + 8] == bytes.fromhex("0123456789abcdef")
    star = both(b"r\t0\tchr1\t1\t0\t*\t*\t0\t0\t*\t*")
    assert len(star) == 4 + 32 + 2 and struct.unpack_from("<i", star, 4 + 16)[0] == 0
    cig = both(b"r\t0\tchr1\t1\t0\t1M2I3D4N5S6H7P8=9X\t*\t0\t0\t" + b"A" * 25 + b"\t*")
    assert struct.unpack_from("<9I", cig, 4 + 32 + 2) == tuple((i + 1) << 4 | i for i in range(9))
    for rnext, want in ((b"=", 0), (b"*", -1), (b"chr2", 1), (b"chr1", 0)):
        rec = both(b"r\t0\tchr1\t1\t0\t1M\t%s\t9\t-300\tA\t*" % rnext)
        assert struct.unpack_from("<iii", rec, 4 + 20) == (want, 8, -300)
    assert struct.unpack_from("<i", both(b"r\t0\t*\t0\t0\t*\t=\t0\t0\t*\t*"), 4 + 20)[0] == -1   # = takes the record's refID


def test_float_tags():
    for txt in (b"0.000", b"0.500", b"1.000", b"-0.125", b"0.333", b"123456.789", b"7", b"0.1", b"999999999999999", b"0.0000000000000000000001"):
        rec = both(R2 + b"\tPA:f:" + txt)
        assert rec[4 + 35:] == b"PAf" + struct.pack("<f", float(txt))           # strtod, then float32


LINES = [R1, R2, R3, R2 + b"\tXY:i:-32769\tXZ:Z:", b"q\t1024\tchr2\t77\t255\t10M\tchr1\t1\t-5\tACGTACGTAC\tABCDEFGHIJ\tPA:f:0.125\tYD:A:f"]


def test_decode_gives_the_line_back():
    refs = M.header_refs(HDR)
    for line in LINES:
        assert M.decode_record(M.encode_record(line, IDS)[4:], refs) == line
    hp, body = M.encode_sam(HDR + b"\n".join(LINES) + b"\n")
    text, refs2, recs = M.split_payload(hp + body)
    assert text == HDR and refs2 == refs and [M.decode_record(r, refs) for r in recs] == LINES


REFUSED = [
    (R1 + b"\tfoo", M.E_TAG), (R1 + b"\tXX:H:1AE3", M.E_TAG), (R1 + b"\tXX:B:c,1,2", M.E_TAG), (R1 + b"\tXX:A:ab", M.E_TAG), (R1 + b"\tXX:i:", M.E_TAG),
    (R1 + b"\tXX:i:1x", M.E_TAG), (R1 + b"\tXX:f:1e5", M.E_TAG), (R1 + b"\tXX:f:1.", M.E_TAG), (R1 + b"\tXX:f:1000000000000000", M.E_TAG), (R1 + b"\t", M.E_TAG),
    (R1 + b"\tX:i:1", M.E_TAG),
    (R1 + b"\tXX:i:%d" % (1 << 32), M.E_INT), (R1 + b"\tXX:i:%d" % (-(1 << 31) - 1), M.E_INT), (R1 + b"\tXX:i:99999999999999999999", M.E_INT),
    (b"n" * 255 + R2[2:], M.E_NAME),
    (b"r\t0\tchr1\t1\t0\t" + b"1M1I" * 32768 + b"\t*\t0\t0\t*\t*", M.E_CIGAR),
    (R1.replace(b"chr1", b"chr3"), M.E_REF), (R1.replace(b"=", b"chrX"), M.E_REF),
    (R1.replace(b"IIIII", b"IIII"), M.E_QUAL), (b"r\t0\tchr1\t1\t0\t*\t*\t0\t0\t*\tII", M.E_QUAL),
    (b"r\t0\tchr1\t1\t0\t*\t*\t0\t0\t*", M.E_LINE), (b"r\tx\tchr1\t1\t0\t*\t*\t0\t0\t*\t*", M.E_LINE), (b"r\t0\tchr1\t1\t0\t3\t*\t0\t0\t*\t*", M.E_LINE),
    (b"r\t0\tchr1\t1\t0\t3Q\t*\t0\t0\t*\t*", M.E_LINE), (b"r\t65536\tchr1\t1\t0\t*\t*\t0\t0\t*\t*", M.E_LINE), (b"r\t0\tchr1\t\t0\t*\t*\t0\t0\t*\t*", M.E_LINE),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_refusals(k):
    line, code = REFUSED[k]
    with pytest.raises(M.Refused) as e:
        M.encode_record(line, IDS)
    assert e.value.code == code
    # the records before the refused one are returned, it is named by its 0-based index, nothing behind it is taken
    text = R1 + b"\n" + R2 + b"\n" + line + b"\n" + R3 + b"\n"
    assert M.encode_body(text, IDS) == (B1 + B2, (2, code))
    assert lib_encode(text) == (B1 + B2, 2, code)


def test_a_name_of_254_bytes_is_taken():
    rec = both(b"n" * 254 + R2[2:])
    assert rec[4 + 8] == 255 and len(rec) == 4 + 32 + 255


def test_block_framing():
    hp = M.encode_header(HDR)
    body = M.encode_body(b"".join(l + b"\n" for l in LINES) * 500, IDS)[0]
    assert len(body) > 2 * M.BGZF_BLOCK
    data = M.bgzf_blocks(hp, body)
    sizes = []
    assert M.bgzf_payload(data, sizes) == hp + body
    n_full = len(body) // M.BGZF_BLOCK
    assert sizes == [len(hp)] + [M.BGZF_BLOCK] * n_full + [len(body) % M.BGZF_BLOCK, 0]
    assert data.endswith(M.BGZF_EOF) and len(M.BGZF_EOF) == 28
    stored = M.bgzf_block(bytes(range(256)))
    assert len(stored) == 256 + 31 and zlib.decompress(stored, 31) == bytes(range(256))
    with pytest.raises((AssertionError, zlib.error)):
        M.bgzf_members(data[:100] + bytes([data[100] ^ 1]) + data[101:])          # a damaged member does not pass
