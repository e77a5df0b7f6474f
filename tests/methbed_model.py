"""Independent model of the per-cytosine methylation BED (`biscuit pileup` -> `biscuit vcf2bed -t TYPE -k K`, optionally -> `biscuit mergecg`, all other
settings at their defaults, one sample) applied to the aligner's own output: SAM text and the FASTA -> the text of --meth-bed's file.  Plain
Python; it shares nothing with the product's meth.c or k_msite.hip and imports nothing from biscuit_amd.  The counters, the site rule and the
beta in thousandths are those of tests/meth_model.py (the records and columns `biscuit pileup` counts); DESIGN.md section 7 has the rule:

  sites     a reference C or G outside N holes with ret + conv > 0 that is callable (meth_model.callable_site)
  class     pileup's CX (bisc_utils.c:33-72) over the five bases i - 2 .. i + 2 read on the cytosine's own strand (for a G: the reverse complement):
            CN when one of them is N or beyond the contig's ends, else CG when the next base is G, else CHG when the one after it is G, else CHH.
            (meth_model.context looks at one neighbour only: that is the context of the conversion table's columns, not this one)
  type      cg keeps CG; ch keeps CHG and CHH; c keeps every site, CN included (vcf2bed.c: the CX field against the type)
  coverage  then a site is kept when ret + conv >= K (vcf2bed -k, default 1)
  line      name, i, i + 1, beta as d.ddd (meth_model.milli: %1.3f of the VCF's %1.3f, which changes nothing), ret + conv
  merged    (mergecg.c:90-137, 189-221) a kept G at i + 1 goes into the line of a kept C at i; a C line ends at i + 2 whether or not a G joined it,
            a G that found no C begins at i - 1; M = (int)(rintf(bC * nC) + rintf(bG * nG)) with b the beta as printed read back as a double, the
            product in double, rintf of it as a float, an absent side 0; the line: name, beg, end, %1.3f of M / cov, cov = nC + nG, C:b:n,G:b:n
            with `.:0` for an absent side
  order     contigs in the order of the SAM header's @SQ lines (the first of two equal names counts), those without a line behind the others in
            the FASTA's order; positions ascending
"""
import struct
import meth_model as M
from meth_model import read_fasta                       # noqa: F401

CLASSES = ["CG", "CHG", "CHH", "CN"]
TYPES = {"cg": ("CG",), "ch": ("CHG", "CHH"), "c": ("CG", "CHG", "CHH", "CN")}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def cx_class(seq, i):
    """pileup's CX of the C or G at i of the contig seq"""
    five = [seq[k].upper() if 0 <= k < len(seq) else "N" for k in range(i - 2, i + 3)]
    if seq[i].upper() == "G":
        five = [_COMP.get(b, "N") for b in reversed(five)]
    if any(b not in "ACGT" for b in five):
        return "CN"
    if five[3] == "G":
        return "CG"
    if five[4] == "G":
        return "CHG"
    return "CHH"


def f32(x):
    """the float nearest to the double x (ties to even), as a double"""
    return struct.unpack("f", struct.pack("f", x))[0]


def rintf(x):
    """rintf of the float x in the default rounding mode: to the nearest integer, ties to even"""
    return float(round(x))


def merged_count(ret_c, n_c, ret_g, n_g):
    """mergecg.c:116-118"""
    def side(ret, n):
        if n == 0:
            return 0.0
        beta = float("%d.%03d" % divmod(M.milli(ret, n), 1000))               # atof of the printed beta
        return rintf(f32(beta * float(n)))
    return int(f32(side(ret_c, n_c) + side(ret_g, n_g)))


def beta_text(ret, n):
    return "%d.%03d" % divmod(M.milli(ret, n), 1000)


def contig_order(sam_text, refs):
    seen = []
    for l in sam_text.split("\n"):
        if l.startswith("@SQ\t"):
            for f in l.split("\t")[1:]:
                if f.startswith("SN:"):
                    if f[3:] in refs and f[3:] not in seen:
                        seen.append(f[3:])
                    break
        elif l and not l.startswith("@"):
            break
    return seen + [n for n in refs if n not in seen]


def kept_sites(cnt, seq, typ, min_cov):
    """-> {i: (base, ret, n, class)} of the contig's kept sites"""
    out = {}
    for i, c in enumerate(cnt):
        b = seq[i].upper()
        if b not in "CG" or c[M.RET] + c[M.CONV] == 0 or not M.callable_site(*c):
            continue
        cls = cx_class(seq, i)
        if cls in TYPES[typ] and c[M.RET] + c[M.CONV] >= min_cov:
            out[i] = (b, c[M.RET], c[M.RET] + c[M.CONV], cls)
    return out


def bed_lines(cnt, refs, order, typ="cg", min_cov=1, merge=False):
    """-> the file's lines, and per line what it is made of: (contig, i of the C or of the lone G, has C, has G, class)"""
    if merge and typ != "cg":
        raise ValueError("mergecg joins CpGs: type cg only")
    lines, what = [], []
    for name in order:
        seq = refs[name]
        kept = kept_sites(cnt[name], seq, typ, min_cov)
        for i in sorted(kept):
            b, ret, n, cls = kept[i]
            if not merge:
                lines.append("%s\t%d\t%d\t%s\t%d\n" % (name, i, i + 1, beta_text(ret, n), n))
                what.append((name, i, b == "C", b == "G", cls))
            elif b == "C":
                g = kept.get(i + 1)
                g = g if g is not None and g[0] == "G" else None
                rg, ng = (g[1], g[2]) if g else (0, 0)
                m = merged_count(ret, n, rg, ng)
                lines.append("%s\t%d\t%d\t%s\t%d\tC:%s:%d,G:%s\n" % (name, i, i + 2, beta_text(m, n + ng), n + ng, beta_text(ret, n), n,
                                                                  "%s:%d" % (beta_text(rg, ng), ng) if g else ".:0"))
                what.append((name, i, True, g is not None, cls))
            else:
                p = kept.get(i - 1)
                if p is not None and p[0] == "C":
                    continue                                                    # it went into the C's line
                m = merged_count(0, 0, ret, n)
                lines.append("%s\t%d\t%d\t%s\t%d\tC:.:0,G:%s:%d\n" % (name, i - 1, i + 1, beta_text(m, n), n, beta_text(ret, n), n))
                what.append((name, i, False, True, cls))
    return lines, what


def process(sam_text, refs, typ="cg", min_cov=1, merge=False):
    """-> (the file's text, what each line is made of, seen)"""
    cnt, seen = M.counts(sam_text, refs)
    lines, what = bed_lines(cnt, refs, contig_order(sam_text, refs), typ, min_cov, merge)
    return "".join(lines), what, seen
