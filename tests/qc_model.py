"""Independent model of `biscuit qc` (src/qc.c:112-179) applied to the aligner's own output: SAM text plus the FASTA -> the seven tables'
text and the raw counters.  Plain Python, written from process_qc, bsstrand_func (src/bsstrand.c:60-168), cinread_func (src/cinread.c:50-187),
bsconv_func (src/bsconv.c:63-109), get_bsstrand / infer_bsstrand / fivenuc_context (src/bisc_utils.c) and the formatters (src/qc.c:29-110).
It shares nothing with the product's qc.c or k_qc.hip and imports nothing from biscuit_amd.

Per record, in file order:
  all_tot += 1; MAPQ >= 40: q40_tot += 1 and cinread twice (targets CG, CH; unmapped and secondary records skipped)
  not secondary: mapq[61 if unmapped else MAPQ] += 1; proper and MAPQ >= 40 and 0 <= TLEN <= 1000: isize[TLEN] += 1;
                 paired and proper and MAPQ >= 40: bsconv totals (unmapped and QC-fail records add nothing)
  mapped: nC2T / nG2A over all M columns -> inferred class (f, r, conflict, unknown; min / max is an INTEGER division, so conflict is
          a tie); confusion[tag * 4 + inferred] += 1; strandcnt[(no 0x40) * 8 + reverse * 4 + tag] += 1, tag from YD (f 0, r 1, c 2, u 3)
The walks: M/=/X columns; I, S and H advance the read position, D the reference.  The read is taken WHOLE: a record printed with hard clips
or without SEQ takes the read from a sibling record (or from `reads`), oriented like itself -- positions are those of the original read
(cinread.c:176-179 says so), and no base beyond SEQ is looked at (the tool indexes past SEQ there: a stated difference).
  strand: YD f -> 0, r -> 1, else 0 if nC2T >= nG2A else 1
  strand 0: reference C columns, next = ref[r + 1]; strand 1: reference G columns, next = complement of ref[r - 1]; a base outside the contig
  or not ACGT is N.  CG: next == G; CH: anything else, N included.  retained: read C (G), converted: read T (A), anything else not printed.
  position = qpos (forward record) or l_read - qpos (reverse); positions >= 301 dropped (the tool writes past its array at 301: a stated
  difference).  Conversion totals: bucket = next in ACGT.
"""
from bsconv_model import read_fasta, parse_cigar, COMP, revcomp      # noqa: F401

N_MAPQ, ISIZE, READ_LEN = 61, 1000, 301
TAGS = {"f": 0, "r": 1, "c": 2, "u": 3}
SUFFIXES = ["_mapq_table.txt", "_dup_report.txt", "_strand_table.txt", "_totalReadConversionRate.txt", "_CpGRetentionByReadPos.txt",
            "_CpHRetentionByReadPos.txt", "_isize_table.txt"]


class Counters:
    def __init__(self):
        self.all_tot = self.all_dup = self.q40_tot = self.q40_dup = self.n_isize = 0
        self.mapq = [0] * (N_MAPQ + 1)
        self.isize = [0] * (ISIZE + 1)
        self.strandcnt = [0] * 16
        self.confusion = [0] * 16
        self.conv = [0] * 8                                                          # CpA_R, CpA_C, CpC_R ..
        self.readpos = [[[[0, 0] for _ in range(READ_LEN)] for _ in range(2)] for _ in range(2)]      # [CG, CH][read][pos][C, R]
        # what the tests ask about the input itself
        self.seen = dict(reverse=0, read2=0, yd_u=0, below40=0, q40=0, S=0, I=0, D=0, H=0, pos_gt150=0, secondary=0)

    def flat(self):
        """the column counts in the order of bsx_qc_counts_t"""
        out = []
        for a in self.readpos:
            for b in a:
                for c in b:
                    out += c
        return out + self.conv + self.confusion


def _tag(fields, name):
    for f in fields[11:]:
        if f.startswith(name + ":"):
            return f[5:]
    return None


def _base(ref, r):
    if 0 <= r < len(ref):
        b = ref[r].upper()
        return b if b in COMP else "N"
    return "N"


def whole_read(fields, by_read, reads):
    """the whole read oriented like the record"""
    flag = int(fields[1])
    ops = parse_cigar(fields[5])
    if fields[9] != "*" and not any(op == "H" for _, op in ops):
        return fields[9].upper()
    key = (fields[0], flag & 0xc0)
    if reads is not None and key in reads:
        s = reads[key].upper()
        return revcomp(s) if flag & 0x10 else s
    for other in by_read.get(key, []):
        if other[9] != "*" and (other[5] == "*" or not any(op == "H" for _, op in parse_cigar(other[5]))):
            return other[9].upper() if (int(other[1]) & 0x10) == (flag & 0x10) else revcomp(other[9])
    raise ValueError("no record with the whole sequence of " + fields[0])


def columns(ref, pos1, cigar, seq):
    """(reference index, read position, reference base, read base) of every M column"""
    rpos, qpos = pos1 - 1, 0
    for n, op in parse_cigar(cigar):
        if op in "M=X":
            for j in range(n):
                yield rpos + j, qpos + j, _base(ref, rpos + j), seq[qpos + j]
            rpos += n
            qpos += n
        elif op in "ISH":
            qpos += n
        elif op in "DN":
            rpos += n
        else:
            raise ValueError("unknown CIGAR operation " + op)


def infer(nC2T, nG2A):
    """bsstrand.c:115-132 -> 0 f, 1 r, 2 conflict, 3 unknown"""
    if nC2T == 0 and nG2A == 0:
        return 3
    s = min(nG2A, nC2T) // max(nG2A, nC2T)
    if nC2T > nG2A:
        return 0 if (nG2A == 0 or s <= 0.5) else 2
    return 1 if (nC2T == 0 or s <= 0.5) else 2


def process(sam_text, refs, reads=None):
    """-> Counters over every record of the SAM text; reads: optional {(QNAME, FLAG & 0xc0): the read as sequenced}"""
    lines = [l.split("\t") for l in sam_text.split("\n") if l and not l.startswith("@")]
    by_read = {}
    for f in lines:
        by_read.setdefault((f[0], int(f[1]) & 0xc0), []).append(f)
    c = Counters()
    for f in lines:
        flag, mapq, tlen = int(f[1]), int(f[4]), int(f[8])
        c.all_tot += 1
        if flag & 0x400:
            c.all_dup += 1
        if mapq >= 40:
            c.q40_tot += 1
            if flag & 0x400:
                c.q40_dup += 1
        if not flag & 0x100:
            if flag & 0x4:
                c.mapq[N_MAPQ] += 1
            else:
                c.mapq[mapq] += 1
            if (flag & 0x2) and mapq >= 40 and 0 <= tlen <= ISIZE:
                c.n_isize += 1
                c.isize[tlen] += 1
        else:
            c.seen["secondary"] += 1
        if flag & 0x4:
            continue
        ref = refs[f[2]]
        seq = whole_read(f, by_read, reads)
        cols = list(columns(ref, int(f[3]), f[5], seq))
        nC2T = sum(1 for _, _, rb, qb in cols if rb == "C" and qb == "T")
        nG2A = sum(1 for _, _, rb, qb in cols if rb == "G" and qb == "A")
        yd = _tag(f, "YD")
        tag = TAGS.get(yd, 3)
        c.confusion[tag * 4 + infer(nC2T, nG2A)] += 1
        c.strandcnt[(0 if flag & 0x40 else 1) * 8 + (1 if flag & 0x10 else 0) * 4 + tag] += 1
        c.seen["reverse"] += 1 if flag & 0x10 else 0
        c.seen["read2"] += 1 if flag & 0x80 else 0
        c.seen["yd_u"] += 1 if yd == "u" else 0
        c.seen["below40" if mapq < 40 else "q40"] += 1
        for op in "SIDH":
            c.seen[op] += 1 if any(o == op for _, o in parse_cigar(f[5])) else 0
        do_cin = mapq >= 40 and not flag & 0x100
        do_bsc = do_cin and not flag & 0x400 and not flag & 0x200 and (flag & 0x1) and (flag & 0x2)
        if not do_cin:
            continue
        strand = 0 if yd == "f" else 1 if yd == "r" else (0 if nC2T >= nG2A else 1)
        l_read = len(seq)
        for r, qpos, rb, qb in cols:
            if rb != ("G" if strand else "C"):
                continue
            nxt = COMP.get(_base(ref, r - 1), "N") if strand else _base(ref, r + 1)
            ret = qb == rb
            conv = qb == ("A" if strand else "T")
            if not ret and not conv:
                continue
            if do_bsc and nxt in "ACGT":
                c.conv["ACGT".index(nxt) * 2 + (1 if conv else 0)] += 1
            idx = l_read - qpos if flag & 0x10 else qpos
            if idx < READ_LEN:
                c.readpos[0 if nxt == "G" else 1][1 if flag & 0x80 else 0][idx][0 if conv else 1] += 1
                if idx > 150:
                    c.seen["pos_gt150"] += 1
    return c


def _rate(a, b):
    if a + b == 0:
        return "-nan"      # 0.0 / 0.0 through printf("%.8lf") on this platform, as the tool prints it
    return "%.8f" % (a / (a + b))


def files(c, paired):
    """suffix -> text, as format_* of src/qc.c write them"""
    out = {}
    t = "BISCUITqc Mapping Quality Table\nMapQ\tCount\nunmapped\t%d\n" % c.mapq[N_MAPQ]
    out["_mapq_table.txt"] = t + "".join("%d\t%d\n" % (i, c.mapq[i]) for i in range(N_MAPQ))
    out["_dup_report.txt"] = ("BISCUITqc Read Duplication Table\nNumber of duplicate reads:\t%d\nNumber of reads:\t%d\n"
                              "Number of duplicate q40-reads:\t%d\nNumber of q40-reads:\t%d\n" % (c.all_dup, c.all_tot, c.q40_dup, c.q40_tot))
    t = "BISCUITqc Strand Table\nStrand Distribution:\nstrand\\BS      BSW (f)      BSC (r)\n"
    for i, row in enumerate(("     R1 (f):   ", "     R1 (r):   ", "     R2 (f):   ", "     R2 (r):   ")):
        t += row + "%-13d\n%-13d\n" % (c.strandcnt[4 * i], c.strandcnt[4 * i + 1])
    out["_strand_table.txt"] = t
    out["_totalReadConversionRate.txt"] = ("BISCUITqc Conversion Rate by Read Average Table\nCpA\tCpC\tCpG\tCpT\n" +
                                           "\t".join(_rate(c.conv[2 * i], c.conv[2 * i + 1]) for i in range(4)) + "\n")
    for k, (suffix, name) in enumerate((("_CpGRetentionByReadPos.txt", "CpG"), ("_CpHRetentionByReadPos.txt", "CpH"))):
        t = "BISCUITqc %s Retention by Read Position Table\nReadInPair\tPosition\tConversion/Retention\tCount\n" % name
        for i in range(2):
            for j in range(READ_LEN):
                for s in range(2):
                    if c.readpos[k][i][j][s] > 0:
                        t += "%d\t%d\t%s\t%d\n" % (i + 1, j, "CR"[s], c.readpos[k][i][j][s])
        out[suffix] = t
    if paired:
        t = "BISCUITqc Insert Size Table\nInsertSize\tFraction\tReadCount\n"
        for i in range(ISIZE + 1):
            if c.isize[i] > 0:
                t += "%d\t%.8f\t%d\n" % (i, c.isize[i] / float(c.n_isize), c.isize[i])
        out["_isize_table.txt"] = t
    return out


def read_fastq(path, which):
    """{(name, which): sequence} of a FASTQ / FASTA file of the tests (names up to the first blank, a trailing /1 or /2 dropped)"""
    out = {}
    with open(path) as f:
        lines = [l.rstrip("\n") for l in f]
    i = 0
    while i < len(lines):
        if lines[i].startswith("@"):
            name, seq = lines[i][1:].split()[0], lines[i + 1]
            i += 4
        elif lines[i].startswith(">"):
            name, seq = lines[i][1:].split()[0], lines[i + 1]
            i += 2
        else:
            i += 1
            continue
        if name.endswith("/1") or name.endswith("/2"):
            name = name[:-2]
        out[(name, which)] = seq
    return out
