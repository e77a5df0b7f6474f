"""tests/markdup_model.py on hand-written records: one assertion per clause of the --markdup rule (include/bsx.h)."""
import markdup_model as M

HEAD = "@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chr2\tLN:1000\n"


def rec(name, flag, contig="chr1", pos=100, cigar="50M", yd="f"):
    seq = "*" if flag & 0x100 else "A" * 50
    return "\t".join([name, str(flag), contig, str(pos), "60", cigar, "=", "300", "0", seq, "*", "NM:i:0", "YD:A:" + yd])


def unplaced(name, flag):
    return "\t".join([name, str(flag | 0x4), "*", "0", "0", "*", "*", "0", "0", "A" * 50, "*", "YD:A:f"])


def pair(name, r1=None, r2=None):
    """both ends forward/reverse at fixed places unless given"""
    return [r1 or rec(name, 0x41 | 0x20), r2 or rec(name, 0x81 | 0x10, pos=300)]


def dups(templates):
    text = HEAD + "\n".join(l for t in templates for l in t) + "\n"
    d, out, n, n_keyed = M.process(text)
    flagged = {f[0] for f in (l.split("\t") for l in out.split("\n") if l and l[0] != "@") if int(f[1]) & 0x400}
    assert flagged == {M.names(text)[i] for i in d}
    # nothing but the flag changes, and only on duplicates
    for a, b in zip(text.split("\n"), out.split("\n")):
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:1] + fa[2:] == fb[:1] + fb[2:] and (a == b or int(fb[1]) == int(fa[1]) | 0x400)
    return sorted(d)


def test_u5_forward_leading_soft_hard_and_both():
    assert M.u5(100, "50M", 0) == 100
    assert M.u5(100, "7S43M", 0) == 93
    assert M.u5(100, "7H43M", 0) == 93
    assert M.u5(100, "3H4S43M5S", 0) == 93                   # trailing clips do not move a forward 5' end
    assert M.u5(3, "7S43M", 0) == -4                         # it may be negative
    assert M.u5(100, "*", 0) == 100


def test_u5_reverse_trailing_clips_with_a_deletion_and_an_insertion():
    assert M.u5(100, "50M", 1) == 149
    assert M.u5(100, "20M2D10M3I17M", 1) == 100 + 49 - 1     # reflen = 20 + 2 + 10 + 17: D counts, I does not
    assert M.u5(100, "20M2D10M3I12M5S", 1) == 100 + 44 - 1 + 5
    assert M.u5(100, "6S20M2D10M3I12M2S3H", 1) == 100 + 44 - 1 + 5   # leading clips do not move a reverse 5' end
    assert M.u5(980, "40M10S", 1) == 1029                    # it may lie beyond the contig's end


def test_soft_clipped_copy_equals_its_original():
    a = pair("a")
    b = pair("b", r1=rec("b", 0x41 | 0x20, pos=112, cigar="12S38M"))
    assert dups([a, b]) == [1]
    c = pair("c", r2=rec("c", 0x81 | 0x10, pos=300, cigar="40M6S4H"))      # reverse end: 300 + 40 - 1 + 10 = 349 = 300 + 50 - 1
    assert dups([a, c]) == [1]


def test_same_coordinates_other_strand():
    a = [rec("a", 0, pos=100)]
    b = [rec("b", 0x10, pos=51)]                             # reverse, u5 = 51 + 50 - 1 = 100 as well
    assert M.end_key(a[0].split("\t"))[1] == M.end_key(b[0].split("\t"))[1] == 100
    assert dups([a, b]) == []


def test_same_coordinates_other_yd():
    assert dups([[rec("a", 0, yd="f")], [rec("b", 0, yd="r")]]) == []
    assert dups([[rec("a", 0, yd="r")], [rec("b", 0, yd="r")]]) == [1]


def test_read_1_and_read_2_exchanged():
    a = pair("a")
    b = [rec("b", 0x41 | 0x10, pos=300), rec("b", 0x81 | 0x20)]      # the same two ends, the other way round
    assert dups([a, b]) == []
    assert dups([a, b, pair("c")]) == [2]


def test_one_end_placed_against_both_placed():
    a = pair("a")
    b = [rec("b", 0x41 | 0x8), unplaced("b", 0x81)]
    c = [rec("c", 0x41 | 0x8), unplaced("c", 0x81)]
    assert dups([a, b]) == []
    assert dups([a, b, c]) == [2]                            # two pairs with the same single placed end are equal
    assert dups([b, [rec("s", 0)]]) == []                    # ... but a single read is never compared against a pair


def test_no_end_placed_twice_is_never_flagged():
    a = [unplaced("a", 0x41 | 0x8), unplaced("a", 0x81 | 0x8)]
    b = [unplaced("b", 0x41 | 0x8), unplaced("b", 0x81 | 0x8)]
    assert dups([a, b, [unplaced("c", 0)], [unplaced("d", 0)]]) == []
    assert M.process(HEAD + "\n".join(a + b) + "\n")[2:] == (2, 0)


def test_supplementary_and_secondary_lines_are_all_flagged():
    a = pair("a")
    b = [rec("b", 0x41 | 0x20), rec("b", 0x841 | 0x20, contig="chr2", pos=500, cigar="30H20M"), rec("b", 0x141, pos=700),
         rec("b", 0x81 | 0x10, pos=300)]
    text = HEAD + "\n".join(a + b) + "\n"
    d, out, _, _ = M.process(text)
    assert d == {1}
    flags = [int(l.split("\t")[1]) for l in out.split("\n") if l.startswith("b\t")]
    assert len(flags) == 4 and all(f & 0x400 for f in flags)
    assert not any(int(l.split("\t")[1]) & 0x400 for l in out.split("\n") if l.startswith("a\t"))
    # the supplementary and secondary records are not the end's primary record: they do not enter the key
    c = [b[1].replace("b\t", "c\t", 1), b[0].replace("b\t", "c\t", 1), b[3].replace("b\t", "c\t", 1)]
    assert dups([a, c]) == [1]


def test_three_equal_templates():
    assert dups([pair("a"), pair("b"), pair("c")]) == [1, 2]
    assert dups([[rec("a", 0)], [rec("x", 0, pos=101)], [rec("b", 0)], [rec("c", 0)]]) == [2, 3]


def test_overhangs_on_neighbouring_contigs_do_not_meet():
    # chr1 is 1000 long: a reverse end that overhangs its end by 5 and a forward end that overhangs the start of chr2 by ... coincide in
    # concatenated coordinates (1005 = 1000 + 5), and as plain numbers too when written against the other contig
    a = [rec("a", 0x10, contig="chr1", pos=960, cigar="41M5S")]      # u5 = 960 + 41 - 1 + 5 = 1005 on chr1
    b = [rec("b", 0x10, contig="chr2", pos=1, cigar="5M45S")]        # u5 = 1 + 5 - 1 + 45 = 50 on chr2
    c = [rec("c", 0x10, contig="chr2", pos=960, cigar="41M5S")]      # u5 = 1005 on chr2
    assert M.end_key(a[0].split("\t"))[1] == M.end_key(c[0].split("\t"))[1] == 1005
    assert dups([a, b, c]) == []
    f1 = [rec("f1", 0, contig="chr2", pos=1, cigar="5S45M")]         # u5 = -4 on chr2: concatenated 996
    f2 = [rec("f2", 0, contig="chr1", pos=996)]                      # u5 = 996 on chr1
    assert dups([f1, f2]) == []
