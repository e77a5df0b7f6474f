"""Independent model of the BISCUITqc coverage tables (scripts/QC.sh:136-421) applied to the aligner's own output: SAM text, the FASTA and two
optional BED files -> the text of the twelve depth distributions and of the uniformity table.  Plain Python; it shares nothing with the product's
cov.c or k_cov.hip and imports nothing from biscuit_amd.  This is the project's restatement of the script, not a run of bedtools:

  records   every record without 0x4 counts, secondary, supplementary and 0x400 records too (`bedtools genomecov -ibam`); class `all` is every
            such record, class `q40` those with MAPQ >= 40 (`samtools view -q 40`)
  depth     +1 on every reference column under an M (=, X) run of the CIGAR; D, N, I, S and H cover nothing (-split breaks blocks at D and N)
  bases     every position of every contig, N runs and contigs without reads included (-bga reports depth 0)
  CpGs      a C at i and a G at i + 1 of one contig (case-insensitive; an N is neither), depth min(depth[i], depth[i + 1]) (`groupby -o min`);
            taken from the FASTA, not from an asset BED
  GC masks  chrom start end, 0-based half-open, further columns ignored; a base counts when it lies in any interval, a CpG when either of its
            bases does.  Deliberate deviations: overlapping intervals and a CpG that straddles two windows count once (bedtools: twice)
  files     depth<TAB>count for every depth with a non-zero count, ascending; a uniformity row where sum(count) > 0 and sum(count * depth) > 0:
            mu = float(sum(count * depth)) / float(sum(count)), sigma = sqrt(sum(count * (depth - mu)^2) / sum(count)) accumulated in ascending
            depth, cv = sigma / mu, each as %.6g -- awk's default output format (OFMT = CONVFMT = "%.6g") prints the same for every value
            below 10^6 (an integral value prints as an integer either way)
"""
import gzip
import math
from bsconv_model import read_fasta, parse_cigar      # noqa: F401

NAMES = ["all_base", "all_cpg", "q40_base", "q40_cpg", "all_base_topgc", "all_cpg_topgc", "q40_base_topgc", "q40_cpg_topgc",
         "all_base_botgc", "all_cpg_botgc", "q40_base_botgc", "q40_cpg_botgc"]
TITLES = ["All Bases", "All CpGs", "Q40 Bases", "Q40 CpGs", "All Top GC Bases", "All Top GC CpGs", "Q40 Top GC Bases", "Q40 Top GC CpGs",
          "All Bot GC Bases", "All Bot GC CpGs", "Q40 Bot GC Bases", "Q40 Bot GC CpGs"]
SUFFIXES = ["_covdist_%s_table.txt" % n for n in NAMES] + ["_cv_table.txt"]


def read_bed(path):
    """[(chrom, start, end)] of a plain or gzip BED file"""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    out = []
    for l in raw.decode().split("\n"):
        f = l.split()
        if not f or f[0].startswith("#") or f[0] in ("track", "browser"):
            continue
        out.append((f[0], int(f[1]), int(f[2])))
    return out


def depths(sam_text, refs):
    """{contig: ([depth of all], [depth of q40])} over every contig of refs"""
    dep = {name: ([0] * len(seq), [0] * len(seq)) for name, seq in refs.items()}
    for l in sam_text.split("\n"):
        if not l or l.startswith("@"):
            continue
        f = l.split("\t")
        flag, mapq = int(f[1]), int(f[4])
        if flag & 0x4:
            continue
        a, q = dep[f[2]]
        r = int(f[3]) - 1
        for n, op in parse_cigar(f[5]):
            if op in "M=X":
                for j in range(r, r + n):
                    a[j] += 1
                    if mapq >= 40:
                        q[j] += 1
                r += n
            elif op in "DN":
                r += n
            elif op not in "ISH":
                raise ValueError("unknown CIGAR operation " + op)
    return dep


def tables(sam_text, refs, top=None, bot=None):
    """-> twelve {depth: count} (four without the masks), in NAMES' order; top / bot: [(chrom, start, end)] or None (both or neither)"""
    assert (top is None) == (bot is None)
    dep = depths(sam_text, refs)
    masks = []
    for bed in ([] if top is None else [top, bot]):
        m = {name: [False] * len(seq) for name, seq in refs.items()}
        for chrom, b, e in bed:
            assert 0 <= b <= e <= len(refs[chrom]), (chrom, b, e)
            m[chrom][b:e] = [True] * (e - b)
        masks.append(m)
    out = [dict() for _ in range(4 + 4 * len(masks))]

    def add(t, d):
        out[t][d] = out[t].get(d, 0) + 1

    for name, seq in refs.items():
        s = seq.upper()
        a, q = dep[name]
        for i in range(len(s)):
            add(0, a[i])
            add(2, q[i])
            for r, m in enumerate(masks):
                if m[name][i]:
                    add(4 + 4 * r, a[i])
                    add(6 + 4 * r, q[i])
            if s[i] == "C" and i + 1 < len(s) and s[i + 1] == "G":
                ma, mq = min(a[i], a[i + 1]), min(q[i], q[i + 1])
                add(1, ma)
                add(3, mq)
                for r, m in enumerate(masks):
                    if m[name][i] or m[name][i + 1]:
                        add(5 + 4 * r, ma)
                        add(7 + 4 * r, mq)
    return out


def cv_row(name, t):
    """the uniformity row of one table, or "" (QC.sh:160-171)"""
    s_cnt = sum(t.values())
    s_cov = sum(c * d for d, c in t.items())
    if not (s_cnt > 0 and s_cov > 0):
        return ""
    mu = float(s_cov) / float(s_cnt)
    var = 0.0
    for d in sorted(t):
        var += float(t[d]) * ((d - mu) * (d - mu))
    sigma = math.sqrt(var / float(s_cnt))
    return "%s\t%.6g\t%.6g\t%.6g\n" % (name, mu, sigma, sigma / mu)


def files(tabs):
    """suffix -> text"""
    out = {}
    cv = "BISCUITqc Uniformity Table\ngroup\tmu\tsigma\tcv\n"
    for i, t in enumerate(tabs):
        out["_covdist_%s_table.txt" % NAMES[i]] = ("BISCUITqc Depth Distribution - %s\ndepth\tcount\n" % TITLES[i] +
                                                   "".join("%d\t%d\n" % (d, t[d]) for d in sorted(t) if t[d]))
        cv += cv_row(NAMES[i], t)
    out["_cv_table.txt"] = cv
    return out
