"""The rule of `--markdup` over SAM text, in plain Python (include/bsx.h, DESIGN.md section 7 state it; this file shares no code with the
product).  A template is a run of consecutive records with one QNAME; its ordinal is its index among the templates of the text.  Each end
(read 2: records with 0x80; read 1: all others) has a primary record, the one with neither 0x100 nor 0x800; the end is placed when that
record lacks 0x4 and then contributes (contig, u5, reverse, YD is r), else None.  A template with no placed end is never a duplicate;
another one is a duplicate when a template with a lower ordinal has the same (end 1, end 2); a single read (no 0x1) has "single" for end 2
and so never equals a pair.  Every record of a duplicate gets 0x400."""
import re

CIGAR = re.compile(r"(\d+)([MIDNSHP=X])")


def u5(pos, cigar, reverse):
    """the unclipped 5' coordinate of a record: 1-based like POS, it may be 0, negative or beyond the contig"""
    ops = [(int(n), op) for n, op in CIGAR.findall(cigar)] if cigar != "*" else []
    if not reverse:
        lead = 0
        for n, op in ops:
            if op not in "SH":
                break
            lead += n
        return pos - lead
    reflen = sum(n for n, op in ops if op in "MDN=X")
    trail = 0
    for n, op in reversed(ops):
        if op not in "SH":
            break
        trail += n
    return pos + reflen - 1 + trail


def end_key(fields):
    """one end's part of the key from its primary record, None when the end is not placed"""
    flag = int(fields[1])
    if flag & 0x4:
        return None
    yd = [x[5:] for x in fields[11:] if x.startswith("YD:A:")]
    rev = 1 if flag & 0x10 else 0
    return (fields[2], u5(int(fields[3]), fields[5], rev), rev, 1 if yd and yd[0] == "r" else 0)


def templates(sam_text):
    """-> (header lines, [[record fields, ...] per template])"""
    head, out, last = [], [], None
    for l in sam_text.split("\n"):
        if not l:
            continue
        if l[0] == "@":
            head.append(l)
            continue
        f = l.split("\t")
        if f[0] != last:
            out.append([])
            last = f[0]
        out[-1].append(f)
    return head, out


def template_key(recs):
    ends, paired = [None, None], False
    for f in recs:
        flag = int(f[1])
        if flag & (0x100 | 0x800):
            continue
        ends[1 if flag & 0x80 else 0] = end_key(f)
        paired = paired or bool(flag & 0x1)
    if ends == [None, None]:
        return None
    return tuple(ends) if paired else (ends[0], "single")      # a single read never equals a pair, not even one whose read 2 is not placed


def process(sam_text):
    """-> (set of duplicate ordinals, the SAM text with 0x400 on their records, templates seen, templates with a key)"""
    head, ts = templates(sam_text)
    first, dups, n_keyed = {}, set(), 0
    for i, recs in enumerate(ts):
        k = template_key(recs)
        if k is None:
            continue
        n_keyed += 1
        if k in first:
            dups.add(i)
            for f in recs:
                f[1] = str(int(f[1]) | 0x400)
        else:
            first[k] = i
    lines = head + ["\t".join(f) for recs in ts for f in recs]
    return dups, "\n".join(lines) + ("\n" if sam_text.endswith("\n") else ""), len(ts), n_keyed


def names(sam_text):
    """the QNAME of every template, by ordinal"""
    return [recs[0][0] for recs in templates(sam_text)[1]]
