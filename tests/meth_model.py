"""Independent model of BISCUITqc's base-averaged conversion table (scripts/QC.sh:423-450: `biscuit pileup` -> `biscuit vcf2bed -e -t c` -> awk)
applied to the aligner's own output: SAM text and the FASTA -> the text of PREFIX_totalBaseConversionRate.txt.  Plain Python; it shares nothing
with the product's meth.c or k_meth.hip and imports nothing from biscuit_amd.  This is the project's restatement of the three tools at their
defaults, in integers, not a run of them (DESIGN.md section 7 has the rule and its derivation):

  records   a record counts with none of 0x4, 0x100, 0x200, 0x400, MAPQ >= 40, SEQ as printed of at least 10 bases, not (0x1 without 0x2), and
            AS >= 40 (a record without AS passes, as in the tool); 0x800 records count.  max_nm and max_retention default to 999999 and never bind
  strand    YD:f 0, YD:r 1, anything else inferred: nC2T = M columns with ref C / read T, nG2A = ref G / read A, over columns of quality >= 20;
            0 when nC2T >= nG2A, else 1
  columns   M (=, X) columns of the CIGAR as printed; q1 = 1-based position in the whole read in the record's orientation and len = the whole
            read's length, hard-clipped bases included in both (the deviation --qc has as well); dropped: quality < 20, q1 <= 3, len < q1 + 3,
            a reference N, and on a 0x80 record the columns inside max(POS, PNEXT) .. min(POS + reflen - 1, PNEXT + mate_reflen - 1), with
            mate_reflen from MC (0 for `*`; the record's own reflen when there is no MC, as in the tool).  No QUAL: every column passes
  counters  at a reference C: strand 0 read C -> ret, read T -> conv; strand 1 read C -> opp_ref, read T -> opp_alt; at a reference G: strand 1
            read G -> ret, read A -> conv; strand 0 read G -> opp_ref, read A -> opp_alt
  sites     a reference C or G with ret + conv > 0 that is callable: opp_alt == 0 or 20 * opp_alt < ret + opp_ref
  context   the next base on the cytosine's own strand: C<forward i + 1>, or C<complement of forward i - 1> for a G; a neighbour that is N or
            beyond the contig's end makes the site CN, which no column of the file has
  beta      milli(ret, ret + conv): what printf("%1.3f") shows of the double quotient, times 1000, stated in integers
  file      per context K sites with the sum S of their milli: -1 when K < 20, else '%.6g' % (S / (1000.0 * K))
"""
from fractions import Fraction
from bsconv_model import read_fasta, parse_cigar      # noqa: F401

TITLE = "BISCUITqc Conversion Rate by Base Average Table\n"
SUFFIX = "_totalBaseConversionRate.txt"
CONTEXTS = ["CA", "CC", "CG", "CT", "CN"]
RECORD_FILTERS = ["unmapped", "secondary", "qcfail", "dup", "mapq", "short", "improper", "as"]
COLUMN_RULES = ["lowq", "end5", "end3", "hole", "overlap"]
MIN_MAPQ, MIN_LEN, MIN_AS, MIN_BQ, END5, END3 = 40, 10, 40, 20, 3, 3
RET, CONV, OPP_REF, OPP_ALT = 0, 1, 2, 3


def milli(r, n):
    """the integer that printf("%1.3f", (double)r / (double)n) shows, times 1000 (0 <= r <= n, n > 0)"""
    m0 = 1000 * r // n
    rem = 1000 * r - m0 * n
    if 2 * rem < n:
        return m0
    if 2 * rem > n:
        return m0 + 1
    # a rational tie: the double quotient lies on one side of it or is it; e = fma(d, n, -r) has the sign of the exact d * n - r
    d = float(r) / float(n)
    e = Fraction(d) * n - r
    if e > 0:
        return m0 + 1
    if e < 0:
        return m0
    return m0 if m0 % 2 == 0 else m0 + 1


def _tags(fields):
    return {t[:2]: t[5:] for t in fields[11:]}


def _reflen(ops):
    return sum(n for n, op in ops if op in "MDN=X")


def record_filter(fields):
    """the name of the first record filter that drops the record, or None"""
    flag, mapq = int(fields[1]), int(fields[4])
    tags = _tags(fields)
    if flag & 0x4:
        return "unmapped"
    if flag & 0x100:
        return "secondary"
    if flag & 0x200:
        return "qcfail"
    if flag & 0x400:
        return "dup"
    if mapq < MIN_MAPQ:
        return "mapq"
    if (0 if fields[9] == "*" else len(fields[9])) < MIN_LEN:
        return "short"
    if (flag & 0x1) and not (flag & 0x2):
        return "improper"
    if "AS" in tags and int(tags["AS"]) < MIN_AS:
        return "as"
    return None


def columns(fields, ref):
    """the M columns of a record -> [(0-based position in the contig, reference base, read base, q1, quality passes)], len"""
    seq, qual = fields[9], fields[10]
    ops = parse_cigar(fields[5])
    total = sum(n for n, op in ops if op in "MIS=XH")
    lead_h = ops[0][0] if ops and ops[0][1] == "H" else 0
    out = []
    x, y = 0, int(fields[3]) - 1
    for n, op in ops:
        if op in "M=X":
            for i in range(n):
                at = x + i - lead_h                                       # hard-clipped bases are never indexed into SEQ or QUAL
                ok = qual == "*" or ord(qual[at]) - 33 >= MIN_BQ
                out.append((y + i, ref[y + i].upper(), seq[at].upper(), x + i + 1, ok))
            x += n
            y += n
        elif op in "DN":
            y += n
        elif op in "ISH":
            x += n
        else:
            raise ValueError("unknown CIGAR operation " + op)
    return out, total


def strand_of(fields, cols):
    yd = _tags(fields).get("YD")
    if yd == "f":
        return 0
    if yd == "r":
        return 1
    n_c2t = sum(1 for _, rb, qb, _, ok in cols if ok and rb == "C" and qb == "T")
    n_g2a = sum(1 for _, rb, qb, _, ok in cols if ok and rb == "G" and qb == "A")
    return 0 if n_c2t >= n_g2a else 1


def counts(sam_text, refs):
    """-> ({contig: [[ret, conv, opp_ref, opp_alt] per position]}, seen): seen counts the records each filter dropped, the columns each rule
    dropped (a column dropped by several rules counts under each), the records that counted and those whose strand was inferred"""
    cnt = {name: [[0, 0, 0, 0] for _ in seq] for name, seq in refs.items()}
    seen = {k: 0 for k in RECORD_FILTERS + COLUMN_RULES + ["counted", "inferred", "supplementary", "reverse", "H", "S", "I", "D"]}
    for l in sam_text.split("\n"):
        if not l or l.startswith("@"):
            continue
        f = l.split("\t")
        why = record_filter(f)
        if why:
            seen[why] += 1
            continue
        flag = int(f[1])
        tags = _tags(f)
        ref = refs[f[2]]
        cols, total = columns(f, ref)
        strand = strand_of(f, cols)
        seen["counted"] += 1
        seen["inferred"] += tags.get("YD") not in ("f", "r")
        seen["supplementary"] += bool(flag & 0x800)
        seen["reverse"] += bool(flag & 0x10)
        for op in "HSID":
            seen[op] += op in f[5]
        lo, hi = 1, 0
        if flag & 0x80:
            ops = parse_cigar(f[5])
            pos, pnext, reflen = int(f[3]), int(f[7]), _reflen(ops)
            mc = tags.get("MC")
            mate = reflen if mc is None else 0 if mc == "*" else _reflen(parse_cigar(mc))
            lo, hi = max(pos, pnext), min(pos + reflen - 1, pnext + mate - 1)
        for p, rb, qb, q1, ok in cols:
            drop = {"lowq": not ok, "end5": q1 <= END5, "end3": total < q1 + END3, "hole": rb not in "ACGT", "overlap": lo <= p + 1 <= hi}
            for k, v in drop.items():
                seen[k] += v
            if any(drop.values()):
                continue
            c = cnt[f[2]][p]
            if rb == "C" and qb in "CT":
                c[(RET if qb == "C" else CONV) if strand == 0 else (OPP_REF if qb == "C" else OPP_ALT)] += 1
            elif rb == "G" and qb in "GA":
                c[(RET if qb == "G" else CONV) if strand == 1 else (OPP_REF if qb == "G" else OPP_ALT)] += 1
    return cnt, seen


def callable_site(ret, conv, opp_ref, opp_alt):
    return opp_alt == 0 or 20 * opp_alt < ret + opp_ref


def context(seq, i):
    """index into CONTEXTS of the C or G at i of the contig seq"""
    s = seq[i].upper()
    if s == "C":
        nb = seq[i + 1].upper() if i + 1 < len(seq) else "N"
    else:
        nb = {"A": "T", "C": "G", "G": "C", "T": "A"}.get(seq[i - 1].upper(), "N") if i > 0 else "N"
    return "ACGT".index(nb) if nb in "ACGT" else 4


def tables(cnt, refs):
    """-> (K[5], S[5], uncallable sites): reported sites and the sum of their milli per context of CONTEXTS"""
    K, S, unc = [0] * 5, [0] * 5, 0
    for name, seq in refs.items():
        for i, c in enumerate(cnt[name]):
            if seq[i].upper() not in "CG" or c[RET] + c[CONV] == 0:
                continue
            if not callable_site(*c):
                unc += 1
                continue
            x = context(seq, i)
            K[x] += 1
            S[x] += milli(c[RET], c[RET] + c[CONV])
    return K, S, unc


def file_text(K, S):
    return TITLE + "CA\tCC\tCG\tCT\n" + "\t".join("-1" if K[x] < 20 else "%.6g" % (float(S[x]) / (1000.0 * float(K[x]))) for x in range(4)) + "\n"


def process(sam_text, refs):
    """-> (the file's text, K, S, uncallable sites, seen)"""
    cnt, seen = counts(sam_text, refs)
    K, S, unc = tables(cnt, refs)
    return file_text(K, S), K, S, unc, seen
