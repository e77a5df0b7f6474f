"""The reference statement of --bam: SAM text -> the uncompressed BAM byte stream -> BGZF blocks, with struct and zlib only.

encode_header / encode_record / encode_body are the rule the device (k_bam.hip) and the host (bam.c) follow byte for byte; bgzf_blocks says how
the payload is cut and framed (the compressed bytes inside a block are the coder's own: only what they inflate to is part of the rule);
bgzf_payload reads a file back, checking every member's framing, CRC and ISIZE on the way.  decode_record prints a record back as its SAM line;
an `f` tag comes back as %.3f -- what the aligner writes -- not as samtools' %g."""
import struct
import zlib

BGZF_BLOCK = 0xff00
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
CIGAR_OPS = "MIDNSHP=X"
SEQ_CODES = "=ACMGRSVTWYHKDBN"

# why a record is refused (the numbers are the library's: include/bsx.h BSX_BAM_E_*)
E_LINE, E_TAG, E_INT, E_NAME, E_CIGAR, E_REF, E_QUAL = 1, 2, 3, 4, 5, 6, 7
REASONS = {E_LINE: "not a SAM record", E_TAG: "field is not XX:T:value with T in A i Z f", E_INT: "integer tag outside -2^31 .. 2^32 - 1",
           E_NAME: "read name longer than 254 bytes", E_CIGAR: "more than 65535 CIGAR operations", E_REF: "RNAME or RNEXT without an @SQ line",
           E_QUAL: "SEQ and QUAL of different lengths"}


class Refused(Exception):
    def __init__(self, code, record=None):
        Exception.__init__(self, "record %s: %s" % (record, REASONS[code]))
        self.code, self.record = code, record


def header_refs(text):
    """(name, length) of every @SQ line of the header text, in its order"""
    refs = []
    for line in text.split(b"\n"):
        if not line.startswith(b"@SQ\t"):
            continue
        sn = ln = None
        for f in line.split(b"\t")[1:]:
            if f.startswith(b"SN:") and sn is None:
                sn = f[3:]
            elif f.startswith(b"LN:") and ln is None:
                ln = int(f[3:])
        if sn is not None:
            refs.append((sn, ln or 0))
    return refs


def ref_ids(refs):
    ids = {}
    for i, (name, _) in enumerate(refs):
        ids.setdefault(name, i)   # the first of two equal names counts
    return ids


def encode_header(text):
    refs = header_refs(text)
    out = [b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, ln in refs:
        out += [struct.pack("<i", len(name) + 1), name, b"\0", struct.pack("<i", ln)]
    return b"".join(out)


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14: return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17: return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20: return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23: return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26: return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def _digits(b):
    return len(b) > 0 and all(48 <= c <= 57 for c in b)


def _int(b, signed=True):
    s = b[1:] if signed and b[:1] in (b"-", b"+") else b
    if not _digits(s) or len(s) > 18:
        raise Refused(E_LINE)
    return int(b)


def _tag(f):
    if len(f) < 5 or f[2:3] != b":" or f[4:5] != b":":
        raise Refused(E_TAG)
    t, v = f[3:4], f[5:]
    if t == b"A":
        if len(v) != 1:
            raise Refused(E_TAG)
        return f[:2] + b"A" + v
    if t == b"Z":
        return f[:2] + b"Z" + v + b"\0"
    if t == b"i":
        s = v[1:] if v[:1] in (b"-", b"+") else v
        if not _digits(s):
            raise Refused(E_TAG)
        if len(s) > 18:
            raise Refused(E_INT)
        x = int(v)
        if x < -(1 << 31) or x > (1 << 32) - 1:
            raise Refused(E_INT)
        if x < 0:
            c, fmt = (b"c", "<b") if x >= -128 else (b"s", "<h") if x >= -32768 else (b"i", "<i")
        else:
            c, fmt = (b"C", "<B") if x <= 255 else (b"S", "<H") if x <= 65535 else (b"I", "<I")
        return f[:2] + c + struct.pack(fmt, x)
    if t == b"f":
        s = v[1:] if v[:1] == b"-" else v
        ip, dot, fp = s.partition(b".")
        if not _digits(ip) or (dot and not _digits(fp)) or len(fp) > 22:
            raise Refused(E_TAG)
        m = int(ip + fp)
        if m >= 10 ** 15:
            raise Refused(E_TAG)
        x = float(m) / float(10 ** len(fp))   # both exact: the quotient is strtod's
        if v[:1] == b"-":
            x = -x
        return f[:2] + b"f" + struct.pack("<f", x)
    raise Refused(E_TAG)


def encode_record(line, ids):
    """one SAM line (no newline) -> the record, block_size included"""
    f = line.split(b"\t")
    if len(f) < 11 or any(len(x) == 0 for x in f[:11]):
        raise Refused(E_LINE)
    name, rname, cig, rnext, seq, qual = f[0], f[2], f[5], f[6], f[9], f[10]
    flag, pos, mapq, pnext, tlen = _int(f[1], False), _int(f[3]), _int(f[4], False), _int(f[7]), _int(f[8])
    if flag > 65535 or mapq > 255 or not -(1 << 31) < pos <= (1 << 31) or not -(1 << 31) < pnext <= (1 << 31) or not -(1 << 31) <= tlen < (1 << 31):
        raise Refused(E_LINE)
    if len(name) > 254:
        raise Refused(E_NAME)
    ops, reflen = [], 0
    if cig != b"*":
        n = 0
        have = False
        for c in cig:
            if 48 <= c <= 57:
                n = n * 10 + (c - 48)
                have = True
                if n >= 1 << 28:
                    raise Refused(E_LINE)
            else:
                k = CIGAR_OPS.find(chr(c))
                if k < 0 or not have:
                    raise Refused(E_LINE)
                ops.append(n << 4 | k)
                if chr(c) in "MDN=X":
                    reflen += n
                n, have = 0, False
        if have:
            raise Refused(E_LINE)
        if len(ops) > 65535:
            raise Refused(E_CIGAR)
    if rname == b"*":
        rid = -1
    elif rname in ids:
        rid = ids[rname]
    else:
        raise Refused(E_REF)
    if rnext == b"=":
        nid = rid
    elif rnext == b"*":
        nid = -1
    elif rnext in ids:
        nid = ids[rnext]
    else:
        raise Refused(E_REF)
    l_seq = 0 if seq == b"*" else len(seq)
    if qual != b"*" and len(qual) != l_seq:
        raise Refused(E_QUAL)
    packed = bytearray((l_seq + 1) // 2)
    for i in range(l_seq):
        k = SEQ_CODES.find(chr(seq[i]))
        packed[i >> 1] |= (15 if k < 0 else k) << (0 if i & 1 else 4)
    q = b"\xff" * l_seq if qual == b"*" else bytes(c - 33 & 255 for c in qual)
    L = reflen
    if flag & 4 or cig == b"*" or L == 0:
        L = 1
    tags = []
    for i, t in enumerate(f[11:]):
        tags.append(_tag(t))
    body = struct.pack("<iiBBHHHiiii", rid, pos - 1, len(name) + 1, mapq, reg2bin(pos - 1, pos - 1 + L), len(ops), flag, l_seq, nid, pnext - 1, tlen)
    body += name + b"\0" + struct.pack("<%dI" % len(ops), *ops) + bytes(packed) + q + b"".join(tags)
    return struct.pack("<i", len(body)) + body


def encode_body(text, ids):
    """whole lines -> (records, None), or (the records before the first refused one, (its 0-based index, code))"""
    out = []
    if text and not text.endswith(b"\n"):
        raise ValueError("whole lines only")
    for i, line in enumerate(text.split(b"\n")[:-1]):
        try:
            out.append(encode_record(line, ids))
        except Refused as e:
            return b"".join(out), (i, e.code)
    return b"".join(out), None


def encode_sam(sam):
    """a whole SAM file (header lines, then records) -> the payload's two parts"""
    at = 0
    while sam[at:at + 1] == b"@":
        at = sam.index(b"\n", at) + 1
    hdr = sam[:at]
    body, bad = encode_body(sam[at:], ref_ids(header_refs(hdr)))
    if bad:
        raise Refused(bad[1], bad[0])
    return encode_header(hdr), body


def bgzf_block(data, raw=None):
    """one member around `data` (raw: its deflate stream; None: zlib's, or stored when that is no smaller)"""
    if raw is None:
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        raw = c.compress(data) + c.flush()
        if len(raw) >= len(data) + 5:
            raw = b"\1" + struct.pack("<HH", len(data), len(data) ^ 0xffff) + data
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(raw) + 25) + raw +
            struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))


def bgzf_blocks(header, body):
    out = [bgzf_block(header[i:i + BGZF_BLOCK]) for i in range(0, len(header), BGZF_BLOCK)]   # the header part ends its block
    out += [bgzf_block(body[i:i + BGZF_BLOCK]) for i in range(0, len(body), BGZF_BLOCK)]
    return b"".join(out) + BGZF_EOF


def bgzf_members(data):
    """the members of a BGZF file as (payload, member bytes); every header field, the CRC and ISIZE are checked"""
    at, out = 0, []
    while at < len(data):
        h = data[at:at + 18]
        assert len(h) == 18 and h[:4] == b"\x1f\x8b\x08\x04", "member magic at %d" % at
        assert h[4:8] == b"\0\0\0\0" and h[8] == 0 and h[9] == 255, "MTIME / XFL / OS at %d" % at
        assert h[10:12] == b"\x06\0" and h[12:14] == b"BC" and h[14:16] == b"\x02\0", "extra field at %d" % at
        size = struct.unpack("<H", h[16:18])[0] + 1
        assert size <= 65536 and at + size <= len(data), "BSIZE at %d" % at
        member = data[at:at + size]
        d = zlib.decompressobj(31)            # gzip framing: zlib checks the CRC and ISIZE itself
        payload = d.decompress(member)
        assert d.eof and d.unused_data == b"", "member at %d is not one whole gzip member" % at
        assert struct.unpack("<II", member[-8:]) == (zlib.crc32(payload) & 0xffffffff, len(payload))
        assert len(payload) <= BGZF_BLOCK
        out.append((payload, member))
        at += size
    return out


def bgzf_payload(data, sizes=None):
    """the joined payload of a BGZF file that ends with the EOF block; sizes (a list) gets every member's payload length"""
    assert data[-28:] == BGZF_EOF, "no EOF block"
    m = bgzf_members(data)
    assert m[-1][0] == b""
    if sizes is not None:
        sizes.extend(len(p) for p, _ in m)
    return b"".join(p for p, _ in m)


def split_payload(payload):
    """(header text, refs, [records without block_size])"""
    assert payload[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", payload, 4)[0]
    text = payload[8:8 + l_text]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", payload, at)[0]
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", payload, at)[0]
        name = payload[at + 4:at + 4 + l_name - 1]
        assert payload[at + 4 + l_name - 1] == 0
        refs.append((name, struct.unpack_from("<i", payload, at + 4 + l_name)[0]))
        at += 8 + l_name
    recs = []
    while at < len(payload):
        n = struct.unpack_from("<i", payload, at)[0]
        recs.append(payload[at + 4:at + 4 + n])
        at += 4 + n
    assert at == len(payload)
    return text, refs, recs


def decode_record(rec, refs):
    """a record (without block_size) -> its SAM line (no newline)"""
    rid, pos, l_name, mapq, _bin, n_cig, flag, l_seq, nid, npos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 0)
    at = 32
    name = rec[at:at + l_name - 1]
    at += l_name
    cig = b"".join(b"%d%c" % (v >> 4, ord(CIGAR_OPS[v & 15])) for v in struct.unpack_from("<%dI" % n_cig, rec, at)) or b"*"
    at += 4 * n_cig
    seq = bytes(ord(SEQ_CODES[rec[at + (i >> 1)] >> (0 if i & 1 else 4) & 15]) for i in range(l_seq)) or b"*"
    at += (l_seq + 1) // 2
    q = rec[at:at + l_seq]
    qual = b"*" if l_seq == 0 or q == b"\xff" * l_seq else bytes(c + 33 for c in q)
    at += l_seq
    tags = []
    while at < len(rec):
        tag, t = rec[at:at + 2], rec[at + 2:at + 3]
        at += 3
        if t == b"A":
            tags.append(tag + b":A:" + rec[at:at + 1]); at += 1
        elif t == b"Z":
            e = rec.index(b"\0", at)
            tags.append(tag + b":Z:" + rec[at:e]); at = e + 1
        elif t == b"f":
            tags.append(tag + b":f:" + (b"%.3f" % struct.unpack_from("<f", rec, at)[0])); at += 4
        else:
            fmt = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}[t]
            tags.append(tag + b":i:" + (b"%d" % struct.unpack_from(fmt, rec, at)[0])); at += struct.calcsize(fmt)
    rn = b"*" if rid < 0 else refs[rid][0]
    nn = b"*" if nid < 0 else b"=" if nid == rid else refs[nid][0]
    return b"\t".join([name, b"%d" % flag, rn, b"%d" % (pos + 1), b"%d" % mapq, cig, nn, b"%d" % (npos + 1), b"%d" % tlen, seq, qual] + tags)
