"""Independent model of `biscuit bsconv` applied to the aligner's own output: retention / conversion counts by cytosine context (the
ZN:Z tag), the per-record filters and the totals, from SAM text plus the FASTA.  Plain Python over forward coordinates, walking each
record as the tool walks a BAM record (src/bsconv.c:30-190, get_bsstrand / infer_bsstrand / fivenuc_context of src/bisc_utils.c).  It
shares nothing with the product's sam.c or its kernel and imports nothing from biscuit_amd: tests compare the product against it.

The rule, for a mapped record: walk the CIGAR from POS over SEQ as printed; M/=/X columns only; I and S advance the query, D the
reference, H neither (hard-clipped bases are not in SEQ -- the one deliberate difference from the tool, which advances over them).
  strand 0 (YD:A:f): columns whose reference base is C; context = the reference base at rpos+1; retained = read C, converted = read T
  strand 1 (YD:A:r): columns whose reference base is G; context = the complement of the base at rpos-1; retained = read G, converted = read A
  a context base outside the contig or not one of ACGT (an N run of the FASTA) is 'N': the column goes to no printed bucket;
  a column whose own reference base is not C / G (an N run included) is skipped;
  YD:A:u: strand = 0 if nC2T >= nG2A else 1, both counted over all aligned columns (minimum base quality 0).
A secondary record printed without its sequence (SEQ '*') is walked over the read taken from the record of the same read that has
it, oriented like the secondary; that sequence is unclipped, so there H does advance.
"""

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
ORDER = "ACGT"


class Conf:
    def __init__(self, annotate=True, filter_u=False, show_filtered=False, max_cph=-1, max_cpa=-1, max_cpc=-1, max_cpt=-1, max_cpy=-1,
                 max_cph_frac=1.0, max_cpy_frac=1.0):
        self.annotate, self.filter_u, self.show_filtered = annotate, filter_u, show_filtered
        self.max_cph, self.max_cpa, self.max_cpc, self.max_cpt, self.max_cpy = max_cph, max_cpa, max_cpc, max_cpt, max_cpy
        self.max_cph_frac, self.max_cpy_frac = max_cph_frac, max_cpy_frac

    def filters(self):
        return bool(self.filter_u or self.show_filtered or self.max_cph >= 0 or self.max_cpa >= 0 or self.max_cpc >= 0 or self.max_cpt >= 0 or
                    self.max_cpy >= 0 or self.max_cph_frac < 1.0 or self.max_cpy_frac < 1.0)


def read_fasta(path):
    """name -> sequence as written (case kept: the model upper-cases on use, as refcache_getbase_upcase does)"""
    out, name, parts = {}, None, []
    with open(path) as f:
        for line in f:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if name is not None:
                    out[name] = "".join(parts)
                name, parts = line[1:].split()[0], []
            elif name is not None:
                parts.append(line)
    if name is not None:
        out[name] = "".join(parts)
    return out


def parse_cigar(c):
    ops, num = [], ""
    for ch in c:
        if ch.isdigit():
            num += ch
        else:
            ops.append((int(num), ch))
            num = ""
    return ops


def _ctx(ch):
    ch = ch.upper()
    return ch if ch in COMP else "N"


def walk(ref, pos1, cigar, seq, h_advances=False):
    """counts[strand][context letter] = [retained, converted] for both strand hypotheses; ref: the contig, pos1: 1-based POS"""
    counts = [{c: [0, 0] for c in "ACGTN"}, {c: [0, 0] for c in "ACGTN"}]
    rpos, qpos = pos1 - 1, 0      # 0-based from here
    for n, op in parse_cigar(cigar):
        if op in "M=X":
            for j in range(n):
                r = rpos + j
                rb = ref[r].upper() if 0 <= r < len(ref) else "N"
                qb = seq[qpos + j].upper()
                if rb == "C":
                    nb = _ctx(ref[r + 1]) if r + 1 < len(ref) else "N"
                    if qb == "C":
                        counts[0][nb][0] += 1
                    elif qb == "T":
                        counts[0][nb][1] += 1
                elif rb == "G":
                    nb = _ctx(ref[r - 1]) if r - 1 >= 0 else "N"
                    nb = COMP.get(nb, "N")
                    if qb == "G":
                        counts[1][nb][0] += 1
                    elif qb == "A":
                        counts[1][nb][1] += 1
            rpos += n
            qpos += n
        elif op in "IS":
            qpos += n
        elif op == "D" or op == "N":
            rpos += n
        elif op == "H":
            if h_advances:
                qpos += n
        else:
            raise ValueError("unknown CIGAR operation " + op)
    return counts


def strand_of(yd, counts):
    if yd == "f":
        return 0
    if yd == "r":
        return 1
    nC2T = sum(v[1] for v in counts[0].values())
    nG2A = sum(v[1] for v in counts[1].values())
    return 0 if nC2T >= nG2A else 1


def zn_string(retn, conv):
    return "ZN:Z:" + ",".join("C%s_R%dC%d" % (c, retn[c], conv[c]) for c in ORDER)


def revcomp(s):
    return "".join(COMP.get(c, "N") for c in reversed(s.upper()))


def _tag(fields, name):
    for f in fields[11:]:
        if f.startswith(name + ":"):
            return f[5:]
    return None


def _seq_of(fields, lines_by_read):
    """SEQ of the record, or for a record printed without it the read from a sibling record, oriented like this one -> (seq, unclipped)"""
    if fields[9] != "*":
        return fields[9], False
    flag = int(fields[1])
    for other in lines_by_read.get((fields[0], flag & 0xc0), []):
        if other[9] != "*" and (other[5] == "*" or not any(op == "H" for _, op in parse_cigar(other[5]))):
            oflag = int(other[1])
            return (other[9] if (oflag & 0x10) == (flag & 0x10) else revcomp(other[9])), True
    raise ValueError("no record with the sequence of " + fields[0])


def record(fields, refs, conf, lines_by_read=None):
    """one SAM record (list of fields) -> (keep, ZN string or None, retn, conv, filtered) by the tool's rule under conf"""
    flag = int(fields[1])
    retn = {c: 0 for c in ORDER}
    conv = {c: 0 for c in ORDER}
    filt = conf.filters()
    unmapped = bool(flag & 0x4)
    tofilter = False
    counted = False
    if unmapped or (flag & 0x200):
        tofilter = True
    else:
        yd = _tag(fields, "YD")
        if yd == "u" and conf.filter_u:
            tofilter = True
        else:
            seq, unclipped = _seq_of(fields, lines_by_read or {})
            counts = walk(refs[fields[2]], int(fields[3]), fields[5], seq, h_advances=unclipped)
            st = strand_of(yd, counts)
            for c in ORDER:
                retn[c], conv[c] = counts[st][c]
            counted = True
            if filt:
                import numpy as np
                f32 = np.float32
                if conf.max_cpa >= 0 and retn["A"] > conf.max_cpa:
                    tofilter = True
                if conf.max_cpc >= 0 and retn["C"] > conf.max_cpc:
                    tofilter = True
                if conf.max_cpt >= 0 and retn["T"] > conf.max_cpt:
                    tofilter = True
                if conf.max_cph >= 0 and retn["A"] + retn["C"] + retn["T"] > conf.max_cph:
                    tofilter = True
                if conf.max_cpy >= 0 and retn["C"] + retn["T"] > conf.max_cpy:
                    tofilter = True
                if conf.max_cph_frac < 1.0:
                    r_, c_ = retn["A"] + retn["C"] + retn["T"], conv["A"] + conv["C"] + conv["T"]
                    if r_ + c_ > 0 and f32(r_) / f32(r_ + c_) > f32(conf.max_cph_frac):
                        tofilter = True
                if conf.max_cpy_frac < 1.0:
                    r_, c_ = retn["C"] + retn["T"], conv["C"] + conv["T"]
                    if r_ + c_ > 0 and f32(r_) / f32(r_ + c_) > f32(conf.max_cpy_frac):
                        tofilter = True
    if not filt:      # annotate only: mapped records gain ZN, everything passes
        return True, (zn_string(retn, conv) if counted else None), retn, conv, False
    keep = tofilter if conf.show_filtered else not tofilter
    return keep, zn_string(retn, conv), retn, conv, tofilter


def process(sam_text, refs, conf):
    """SAM text (str) -> (output text, totals[8] in the tool's retn_conv_counts order, records seen, records filtered)"""
    lines = sam_text.split("\n")
    by_read = {}
    for l in lines:
        if l and not l.startswith("@"):
            f = l.split("\t")
            by_read.setdefault((f[0], int(f[1]) & 0xc0), []).append(f)
    out, tot, n, nf = [], [0] * 8, 0, 0
    for l in lines:
        if not l or l.startswith("@"):
            out.append(l)
            continue
        f = l.split("\t")
        keep, zn, retn, conv, filtered = record(f, refs, conf, by_read)
        n += 1
        nf += 1 if filtered else 0
        if not keep:
            continue
        for i, c in enumerate(ORDER):
            tot[2 * i] += retn[c]
            tot[2 * i + 1] += conv[c]
        out.append(l + ("\t" + zn if zn else ""))
    return "\n".join(out), tot, n, nf
