"""The reference statement of `--sort` (include/bsx.h): plain Python over SAM text.  A sorted SAM is the model's rewrite of
the unsorted SAM of the same command line: the header with its @HD line first and SO:coordinate in it, every other header line as it is, then
the body's lines -- nothing inside a line changes -- ordered by (rank of RNAME among the header's @SQ lines, POS, FLAG & 0x10), equal keys in
the order the unsorted output has them."""

NO_RANK = 0xffffffff      # RNAME '*' (and a name the header has no @SQ line for): after every contig


def split(text):
    """-> (header lines, body lines), without their newlines"""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    n = 0
    while n < len(lines) and lines[n].startswith("@"):
        n += 1
    return lines[:n], lines[n:]


def ranks(header):
    """RNAME -> 0-based index among the @SQ lines as written (the first of two lines with one name counts)"""
    out, i = {}, 0
    for l in header:
        if l.startswith("@SQ\t"):
            for f in l.split("\t")[1:]:
                if f.startswith("SN:"):
                    if f[3:] != "*":
                        out.setdefault(f[3:], i)
                    break
            i += 1
    return out


def key(line, rk):
    f = line.split("\t")
    return (NO_RANK if f[2] == "*" else rk.get(f[2], NO_RANK), int(f[3]), 1 if int(f[1]) & 0x10 else 0)


def header(lines):
    """@HD first: the header's own (its SO: field set to coordinate, or appended), or a new one"""
    for i, l in enumerate(lines):
        if l == "@HD" or l.startswith("@HD\t"):
            f = l.split("\t")
            had = any(x.startswith("SO:") for x in f[1:])
            f = f[:1] + ["SO:coordinate" if x.startswith("SO:") else x for x in f[1:]] + ([] if had else ["SO:coordinate"])
            return ["\t".join(f)] + lines[:i] + lines[i + 1:]
    return ["@HD\tVN:1.6\tSO:coordinate"] + lines


def process(text):
    """unsorted SAM text -> the sorted SAM text"""
    h, body = split(text)
    rk = ranks(h)
    return "".join(l + "\n" for l in header(h) + sorted(body, key=lambda l: key(l, rk)))
