"""-m gpu: BAM output on the device.  (a) Device.bam_encode (k_bam.hip) against tests/bam_model.py: the hand-worked lines, lines that cross the
scan tiles (4096 bytes) and a line longer than a tile, text that ends exactly at a tile's end, empty text, three trips of the one-workgroup
scan plus one line (and so thirteen workgroups of the line kernel), a 254-byte name, the first refused record for every refusal.  (b)
Device.bgzf_deflate (k_bgzf.hip): zlib must inflate every member back to the payload, at the lengths and contents where the coder takes another
path, with the size bounds that tell a coder with matches and dynamic codes from one without; the same call twice gives the same bytes.  (c) the
HIP command line with --bam: its payload against the model's encoding of its own plain run and against the CPU checker's payload, with --sort
--markdup, and through the emit hook; the device's size against zlib level 1 over the same blocks (profiles/bam_measurements.md has the
measurement the bound comes from)."""
import os
import subprocess
import sys
import zlib
import numpy as np
import pytest
import bam_cases as BC
import bam_model as M
import test_bam_model as TM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "biscuit_amd", "biscuit_align")
CPU = os.path.join(ROOT, "oracle", "oracle_align")
BLOCK = M.BGZF_BLOCK
# device bytes / zlib level 1 bytes over the blocks of the command line's payload, measured once on the MI355X (profiles/bam_measurements.md),
# plus 5 % for later edits to the read simulator: the device's stream is a function of the payload
RATIO_MEASURED = 1.0451      # 80 323 bytes against 76 857 over the 5 blocks (241 586 payload bytes) of the pe150_b0 command line
RATIO_BOUND = RATIO_MEASURED * 1.05


@pytest.fixture(scope="module")
def dev():
    from biscuit_amd.api import Device
    d = Device(0)
    yield d
    d.close()


def line(i, tag=b""):
    return b"read%07d\t%d\tchr%d\t%d\t%d\t20M1I9M\t=\t%d\t%d\tACGTACGTACGTACGTACGTACGTACGTAC\tFFFFFFFFFFFFFFF,,,,:::::FFFFF#\tNM:i:%d\tPA:f:0.%03d\tYD:A:f%s" % (
        i, 99 if i % 3 else 147, 1 + i % 2, 1000 + i * 7, i % 61, 1100 + i * 7, -130 if i % 2 else 130, i % 300 - 3, i % 1000, tag)


def check_encode(dev, text, what):
    want, bad = M.encode_body(text, TM.IDS)
    got, bad_rec, why = dev.bam_encode(TM.HDR, text)
    assert (bad_rec, why) == ((-1, 0) if bad is None else bad), (what, bad_rec, why, bad)
    assert len(got) == len(want), (what, len(got), len(want))
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError("%s: byte %d of %d differs" % (what, at, len(want)))
    return got


def test_encode_hand_worked_lines_and_a_long_name(dev):
    assert check_encode(dev, TM.R1 + b"\n" + TM.R2 + b"\n" + TM.R3 + b"\n", "hand-worked") == TM.B1 + TM.B2 + TM.B3
    check_encode(dev, b"".join(l + b"\n" for l in TM.LINES), "lines")
    check_encode(dev, b"n" * 254 + TM.R2[2:] + b"\n", "254-byte name")
    assert dev.bam_encode(TM.HDR, b"") == (b"", -1, 0)
    for v in (-(1 << 31), -32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536, (1 << 31) - 1, (1 << 32) - 1):
        check_encode(dev, TM.R2 + b"\tXY:i:%d\n" % v, "i:%d" % v)
    for txt in (b"0.000", b"0.333", b"-0.125", b"123456.789", b"999999999999999", b"0.0000000000000000000001"):
        check_encode(dev, TM.R2 + b"\tPA:f:" + txt + b"\n", "f:" + txt.decode())


def test_encode_across_tiles_and_scan_trips(dev):
    body = b"".join(line(i) + b"\n" for i in range(3 * 1024 + 1))                  # three trips of the scan plus one line
    assert len(body) > 100 * 4096
    check_encode(dev, body, "3073 lines")
    long_tag = b"\tZZ:Z:" + b"x" * 9000                                           # a line over more than two tiles: tiles without a newline
    check_encode(dev, line(0) + b"\n" + line(1, long_tag) + b"\n" + line(2) + b"\n", "a long line")
    for total in (4096, 8192, 8192 + 16, 8192 - 1, 8192 + 1):                        # the text ends exactly at a tile's end, and a byte either side
        head = b"".join(line(i) + b"\n" for i in range(20))
        last = line(40, b"\tZZ:Z:" + b"y" * (total - len(head) - len(line(40)) - 7)) + b"\n"
        assert len(head + last) == total
        check_encode(dev, head + last, "text of %d bytes" % total)
    for at in (4095, 4096):                                                          # a newline as the last byte of a tile, and as the first of the next
        first = line(5, b"\tZZ:Z:" + b"z" * (at - len(line(5)) - 6)) + b"\n"
        assert len(first) == at + 1
        check_encode(dev, first + line(6) + b"\n", "newline at byte %d" % at)


@pytest.mark.parametrize("k", range(len(TM.REFUSED)))
def test_encode_reports_the_first_refused_record(dev, k):
    bad_line, code = TM.REFUSED[k]
    lines = [line(i) for i in range(800)]
    lines[700] = TM.REFUSED[(k + 1) % len(TM.REFUSED)][0]                           # a later refused line, in another workgroup: not the one reported
    lines[300] = bad_line
    text = b"".join(l + b"\n" for l in lines)
    got, bad_rec, why = dev.bam_encode(TM.HDR, text)
    assert (bad_rec, why) == (300, code)
    assert got == M.encode_body(b"".join(l + b"\n" for l in lines[:300]), TM.IDS)[0]


def members(data):
    return M.bgzf_members(data)      # framing, CRC32 and ISIZE of every member checked by zlib


def deflate_checked(dev, payload, what):
    out = dev.bgzf_deflate(payload)
    ms = members(out)
    assert b"".join(p for p, _ in ms) == payload, what
    assert [len(p) for p, _ in ms] == [BLOCK] * (len(payload) // BLOCK) + ([len(payload) % BLOCK] if len(payload) % BLOCK else []), what
    assert all(len(m) <= 65536 for _, m in ms)
    assert dev.bgzf_deflate(payload) == out, what + ": the same call twice"
    return [m for _, m in ms]


def coded(member):
    """BTYPE of the member's first deflate block"""
    return member[18] >> 1 & 3


def de_bruijn(k, n):
    """the k^n symbols of a de Bruijn sequence: read linearly, no n-gram occurs twice"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq


def test_deflate_lengths(dev):
    r = np.random.default_rng(7)
    text = b"".join(line(i) + b"\n" for i in range(2000))
    assert dev.bgzf_deflate(b"") == b""
    for n in (1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 7):
        deflate_checked(dev, text[:n], "text, %d bytes" % n)
        ms = deflate_checked(dev, r.integers(0, 256, n, dtype=np.uint8).tobytes(), "random, %d bytes" % n)
        sizes = [BLOCK] * (n // BLOCK) + ([n % BLOCK] if n % BLOCK else [])
        assert [len(m) for m in ms] == [s + 31 for s in sizes] and all(coded(m) == 0 for m in ms)      # stored: 18 + 5 + n + 8


def test_deflate_uses_matches_and_dynamic_codes(dev):
    r = np.random.default_rng(8)
    m, = deflate_checked(dev, b"Q" * BLOCK, "equal bytes")
    assert len(m) < 1024 and coded(m) == 2, len(m)                                   # Huffman alone cannot get under 8160
    four = r.integers(0, 4, BLOCK, dtype=np.uint8)
    m, = deflate_checked(dev, (four * 67 + 3).astype(np.uint8).tobytes(), "four values")
    assert len(m) < 0.30 * BLOCK and coded(m) == 2, len(m)                            # stored and fixed codes: 100 %; Huffman alone: 25 %
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    assert fib[-1] == 17711 and sum(fib) == 46367
    sym = np.repeat(np.arange(22, dtype=np.uint8) * 11 + 5, fib)
    r.shuffle(sym)
    m, = deflate_checked(dev, sym.tobytes(), "Fibonacci frequencies")                # an unlimited tree would be 21 deep
    assert coded(m) == 2 and len(m) < 46367 * 0.4
    m, = deflate_checked(dev, b"\x00" * 1000, "a single byte value")
    assert coded(m) == 2
    deflate_checked(dev, bytes(range(256)), "256 distinct bytes once each")
    m, = deflate_checked(dev, bytes(65 + v for v in de_bruijn(16, 3)), "every trigram once: literals only, no distance code")
    assert coded(m) == 2 and len(m) < 4096 * 0.6
    marker = bytes(r.integers(0, 256, 64, dtype=np.uint8))
    for d in (32768, 32769):                                                         # a repeat at distance exactly 32768, and one at 32769 only
        filler = bytes((r.integers(0, 4, d - 64, dtype=np.uint8) + 250).astype(np.uint8))
        deflate_checked(dev, marker + filler + marker + b"end", "repeat at distance %d" % d)
    # a 600-byte run splits at length 258; between incompressible bytes it is what makes the coded block smaller than the stored one
    head, tail = bytes(r.integers(0, 256, 500, dtype=np.uint8)), bytes(r.integers(0, 256, 500, dtype=np.uint8))
    m, = deflate_checked(dev, head + b"R" * 600 + tail, "a 600-byte run")
    assert coded(m) == 2 and len(m) < 1600 + 31, len(m)


_RUNS = {}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gbam"))
    BC.make_data(d)
    return d


def pair(exe, opts, args, d):
    key = (exe, tuple(opts), tuple(args))
    if key not in _RUNS:
        _RUNS[key] = BC.run_pair(exe, opts, args, d)
    return _RUNS[key]


def test_command_line_payload_is_the_models_and_the_cpu_checkers(data):
    args = dict(BC.CASES)["pe150_b0"]
    sam, bam = pair(HIP, [], args, data)
    payload, n_h = BC.check_bam(bam, sam, "hip")
    csam, cbam = pair(CPU, [], args, data)
    cpay, c_h = BC.check_bam(cbam, csam, "cpu")
    assert payload[n_h:] == cpay[c_h:] and len(payload) - n_h > 2 * BLOCK           # (the headers differ by the @PG line)
    assert bam != cbam                                                               # the compressed bytes are each coder's own
    for piece in ("70001", "5000"):                                                  # the device writer in small pieces: records, block_size fields and blocks
        q = BC.run_raw(HIP, ["--bam"] + args, data, env={"BSX_TUNE": "bam_piece_bytes=" + piece})      # straddle them; the same file byte for byte
        assert q.returncode == 0 and q.stdout == bam, (piece, q.stderr.decode()[-1000:])


def test_command_line_with_sort_and_markdup(data):
    args = dict(BC.CASES)["pe150_b0"]
    sam, bam = pair(HIP, ["--sort", "--markdup"], args, data)
    payload, n_h = BC.check_bam(bam, sam, "hip --sort --markdup")
    assert M.split_payload(payload)[0].startswith(b"@HD\tVN:1.6\tSO:coordinate\n")
    csam, cbam = pair(CPU, ["--sort", "--markdup"], args, data)
    cpay, c_h = BC.check_bam(cbam, csam, "cpu --sort --markdup")
    assert payload[n_h:] == cpay[c_h:]


def test_command_line_through_the_emit_hook(data):
    args = dict(BC.CASES)["pe150_b0"]
    sam, bam = pair(HIP, [], args, data)
    out = data + "/hook.bam"
    e = dict(os.environ, BSX_TUNE="bam_piece_bytes=40000")                           # several pieces: the hook is called for each
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bam_hook_entry.py"), out, "--bam"] + args, cwd=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=600)
    assert p.returncode == 0 and p.stdout == b"", p.stderr.decode()[-2000:]
    got = open(out, "rb").read()
    want, n_hw = BC.check_bam(bam, sam, "hip")
    hooked = M.bgzf_payload(got)
    n_h = len(M.encode_header(M.split_payload(hooked)[0]))
    assert hooked[n_h:] == want[n_hw:]                                               # (the headers differ by the @PG line the program entry adds)
    assert len(M.bgzf_members(got)) == len(M.bgzf_members(bam))


def test_compression_against_zlib_level_1(data):
    args = dict(BC.CASES)["pe150_b0"]
    sam, bam = pair(HIP, [], args, data)
    ms = members(bam)[:-1]
    dev_bytes = sum(len(m) for _, m in ms)
    z_bytes = sum(len(zlib.compress(p, 1)) for p, _ in ms)
    tokens = sum(len(p) for p, _ in ms)
    print("bam compression: payload %d bytes in %d blocks, device %d bytes, zlib level 1 %d bytes, ratio %.4f" % (tokens, len(ms), dev_bytes, z_bytes, dev_bytes / z_bytes))
    assert dev_bytes <= RATIO_BOUND * z_bytes, (dev_bytes, z_bytes, dev_bytes / z_bytes)
