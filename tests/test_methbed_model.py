"""CPU: tests/methbed_model.py (the reference statement of --meth-bed's rule) on hand-worked records, every expected line written out by hand.
A record here is unpaired, MAPQ 60, without qualities: of a read of L bases the columns 4 .. L - 3 count (pileup.c:383), soft-clipped bases
included in L.  A YD:f read counts at reference Cs (C retained, T converted), a YD:r read at reference Gs (G retained, A converted)."""
import pytest
import meth_model as M
import methbed_model as MB

#        0         1         2
#        012345678901234567890123456789
C1 = "TTATACGATCGTATCGAATTATATTAATTA"      # CpGs at 5/6, 9/10, 14/15
C2 = "TTATATTAATATTATAACGA"                # C 17 three from the end, G 18 two from the end
C3 = "TTATATTAATATTATAATAC"                # ends in C
C4 = "GATTATATTAATATTATAAT"                # begins with G
C5 = "TTATACGNTTATATTATAAT"                # N behind the CpG 5/6
C6 = "TTANACGATTATATTATAAT"                # N two before the C 5


def rec(name, ctg, pos0, seq, yd, cigar=None):
    return "\t".join([name, "0", ctg, str(pos0 + 1), "60", cigar or "%dM" % len(seq), "*", "0", "0", seq, "*", "NM:i:0", "AS:i:60", "YD:Z:" + yd])


def sam(refs, recs, header_order=None):
    return "".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(refs[n])) for n in (header_order or list(refs))) + "\n".join(recs) + "\n"


def put(seq, **at):
    """seq with the base at index p replaced: put(s, p5="T")"""
    s = list(seq)
    for k, b in at.items():
        s[int(k[1:])] = b
    return "".join(s)


def text(refs, recs, **kw):
    return MB.process(sam(refs, recs), refs, **kw)[0]


# an f read over c1 0..12 counts at 3..9 (C 5, C 9); an r read over c1 7..22 counts at 10..19 (G 10, G 15)
def f_read(name, c5, c9):
    return rec(name, "c1", 0, put(C1[0:13], p5=c5, p9=c9), "f")


def r_read(name, g10, g15):
    return rec(name, "c1", 7, put(C1[7:23], p3=g10, p8=g15), "r")


def test_the_class_is_the_five_base_one():
    assert [MB.cx_class(C1, i) for i in (5, 6, 9, 10, 14, 15)] == ["CG"] * 6
    assert MB.cx_class("TTCAGTT", 2) == "CHG" and MB.cx_class("TTCATTT", 2) == "CHH" and MB.cx_class("AACTGAA", 4) == "CHG" and MB.cx_class("AAATGAA", 4) == "CHH"
    assert MB.cx_class(C2, 17) == "CG" and MB.cx_class(C2, 18) == "CN" and MB.cx_class(C3, 19) == "CN" and MB.cx_class(C4, 0) == "CN"
    assert MB.cx_class("ACGTT", 1) == "CN" and MB.cx_class("AACGT", 2) == "CG"     # one base, two bases before the C
    assert M.context(C5, 5) == 2                                                   # the conversion table's context of the same C is CG: one neighbour


def test_lone_c_lone_g_and_a_joined_pair():
    refs = {"c1": C1}
    recs = [f_read("a", "C", "T"), f_read("b", "T", "T"), r_read("c", "G", "A")]
    # C 5: 1 of 2; C 9: 0 of 2; G 10: 1 of 1; G 15: 0 of 1
    assert text(refs, recs) == "c1\t5\t6\t0.500\t2\n" "c1\t9\t10\t0.000\t2\n" "c1\t10\t11\t1.000\t1\n" "c1\t15\t16\t0.000\t1\n"
    assert text(refs, recs, merge=True) == ("c1\t5\t7\t0.500\t2\tC:0.500:2,G:.:0\n"          # M = rintf(0.5 * 2) = 1
                                            "c1\t9\t11\t0.333\t3\tC:0.000:2,G:1.000:1\n"      # M = 0 + 1
                                            "c1\t14\t16\t0.000\t1\tC:.:0,G:0.000:1\n")
    assert text(refs, recs, typ="ch") == "" and text(refs, recs, typ="c") == text(refs, recs)
    assert text(refs, recs, min_cov=2) == "c1\t5\t6\t0.500\t2\n" "c1\t9\t10\t0.000\t2\n"


def test_a_g_is_joined_only_when_its_c_passes_k():
    refs = {"c1": C1}
    recs = [f_read("a", "C", "T"), r_read("c", "G", "A"), r_read("d", "A", "A")]
    # C 5: 1 of 1; C 9: 0 of 1; G 10: 1 of 2; G 15: 0 of 2
    assert text(refs, recs, merge=True) == ("c1\t5\t7\t1.000\t1\tC:1.000:1,G:.:0\n"
                                            "c1\t9\t11\t0.333\t3\tC:0.000:1,G:0.500:2\n"      # M = 0 + rintf(0.5 * 2)
                                            "c1\t14\t16\t0.000\t2\tC:.:0,G:0.000:2\n")
    assert text(refs, recs, merge=True, min_cov=2) == ("c1\t9\t11\t0.500\t2\tC:.:0,G:0.500:2\n"
                                                       "c1\t14\t16\t0.000\t2\tC:.:0,G:0.000:2\n")


def test_an_uncallable_c_beside_a_callable_g():
    refs = {"c1": C1}
    # the r read over 3..22 counts at 6..19: T over C 9 (opp_alt 1 against ret + opp_ref 0: uncallable), G over G 6, G 10 and G 15
    recs = [f_read("a", "C", "T"), rec("r", "c1", 3, put(C1[3:23], p6="T"), "r")]
    cnt, _ = M.counts(sam(refs, recs), refs)
    assert cnt["c1"][9] == [0, 1, 0, 1] and not M.callable_site(*cnt["c1"][9]) and cnt["c1"][6] == [1, 0, 1, 0]
    assert text(refs, recs) == "c1\t5\t6\t1.000\t1\n" "c1\t6\t7\t1.000\t1\n" "c1\t10\t11\t1.000\t1\n" "c1\t15\t16\t1.000\t1\n"
    assert text(refs, recs, merge=True) == ("c1\t5\t7\t1.000\t2\tC:1.000:1,G:1.000:1\n"
                                            "c1\t9\t11\t1.000\t1\tC:.:0,G:1.000:1\n"
                                            "c1\t14\t16\t1.000\t1\tC:.:0,G:1.000:1\n")


def test_a_cpg_at_the_contigs_end():
    refs = {"c2": C2}
    # 16M3S over 4..19: of 19 bases the columns 4..16 count, positions 7..19
    recs = [rec("a", "c2", 4, C2[4:20] + "TTT", "f", "16M3S"), rec("b", "c2", 4, C2[4:20] + "TTT", "r", "16M3S")]
    assert text(refs, recs) == "c2\t17\t18\t1.000\t1\n"                        # the G at 18 lacks the base at 20: CN
    assert text(refs, recs, merge=True) == "c2\t17\t19\t1.000\t1\tC:1.000:1,G:.:0\n"
    assert text(refs, recs, typ="c") == "c2\t17\t18\t1.000\t1\n" "c2\t18\t19\t1.000\t1\n"
    assert text(refs, recs, typ="ch") == ""


def test_a_c_at_a_contigs_last_base_and_a_g_at_the_next_ones_first_are_no_cpg():
    refs = {"c3": C3, "c4": C4}
    recs = [rec("a", "c3", 4, C3[4:20] + "TTT", "f", "16M3S"), rec("b", "c4", 0, "TTT" + C4[0:16], "r", "3S16M")]
    assert text(refs, recs) == "" and text(refs, recs, merge=True) == "" and text(refs, recs, typ="ch") == ""
    assert text(refs, recs, typ="c") == "c3\t19\t20\t1.000\t1\n" "c4\t0\t1\t1.000\t1\n"


def test_an_n_within_two_bases():
    refs = {"c5": C5, "c6": C6}
    recs = [rec("a", "c5", 0, C5[0:16].replace("N", "A"), "f"), rec("b", "c5", 0, C5[0:16].replace("N", "A"), "r"),
            rec("c", "c6", 0, C6[0:16].replace("N", "A"), "f"), rec("d", "c6", 0, C6[0:16].replace("N", "A"), "r")]
    # c5: the N at 7 is in the context of the C at 5 and of the G at 6.  c6: the N at 3 is in the context of the C at 5 (3..7), not of the G at 6 (4..8)
    assert text(refs, recs) == "c6\t6\t7\t1.000\t1\n"
    assert text(refs, recs, merge=True) == "c6\t5\t7\t1.000\t1\tC:.:0,G:1.000:1\n"
    assert text(refs, recs, typ="c") == "c5\t5\t6\t1.000\t1\n" "c5\t6\t7\t1.000\t1\n" "c6\t5\t6\t1.000\t1\n" "c6\t6\t7\t1.000\t1\n"


def test_the_merged_count_is_made_in_mergecgs_steps():
    # 501 of 1001 prints 0.500 and 0.5 * 1001 = 500.5 rounds to the even 500, not 501; 1 of 1500 prints 0.001 and 0.001 * 1500 = 1.5 rounds to 2
    assert M.milli(501, 1001) == 500 and MB.merged_count(501, 1001, 0, 0) == 500
    assert M.milli(1, 1500) == 1 and MB.merged_count(1, 1500, 0, 0) == 2 and MB.merged_count(1, 1500, 1, 1500) == 4
    assert MB.merged_count(501, 1001, 501, 1001) == 1000 and MB.merged_count(0, 0, 3, 4) == 3
    refs = {"c1": C1}
    recs = [f_read("a%d" % i, "C" if i < 501 else "T", "T") for i in range(1001)]
    assert text(refs, recs, merge=True) == "c1\t5\t7\t0.500\t1001\tC:0.500:1001,G:.:0\n" "c1\t9\t11\t0.000\t1001\tC:0.000:1001,G:.:0\n"   # 500 / 1001 = 0.4995
    recs = [f_read("a%d" % i, "C" if i < 1 else "T", "T") for i in range(1500)] + [r_read("b%d" % i, "G" if i < 1 else "A", "A") for i in range(1500)]
    # C 5 and G 10: 1 of 1500, C 9 and G 15: 0 of 1500.  The pair 9/10: M = 0 + 2 of 3000 = 0.00067 -> 0.001, where the sum of the retained, 1 of 3000,
    # would print 0.000
    assert text(refs, recs, merge=True) == ("c1\t5\t7\t0.001\t1500\tC:0.001:1500,G:.:0\n"
                                            "c1\t9\t11\t0.001\t3000\tC:0.000:1500,G:0.001:1500\n"
                                            "c1\t14\t16\t0.000\t1500\tC:.:0,G:0.000:1500\n")


def test_a_tie_of_the_beta_goes_to_even():
    refs = {"c1": C1}
    recs = [f_read("a%d" % i, "C" if i < 1 else "T", "C" if i < 3 else "T") for i in range(16)]
    # 1 / 16 = 0.0625 and 3 / 16 = 0.1875 are exact in binary: printf rounds the tie to even
    assert text(refs, recs) == "c1\t5\t6\t0.062\t16\n" "c1\t9\t10\t0.188\t16\n"


def test_contigs_follow_the_headers_sq_lines():
    refs = {"c1": C1, "c2": C2, "c3": C3}
    recs = [f_read("a", "C", "T"), rec("b", "c2", 4, C2[4:20] + "TTT", "f", "16M3S"), rec("c", "c3", 4, C3[4:20] + "TTT", "f", "16M3S")]
    want = {"c1": "c1\t5\t6\t1.000\t1\n" "c1\t9\t10\t0.000\t1\n", "c2": "c2\t17\t18\t1.000\t1\n", "c3": "c3\t19\t20\t1.000\t1\n"}
    assert MB.process(sam(refs, recs), refs, typ="c")[0] == want["c1"] + want["c2"] + want["c3"]
    assert MB.process(sam(refs, recs, header_order=["c2", "c1"]), refs, typ="c")[0] == want["c2"] + want["c1"] + want["c3"]   # no @SQ line: behind the others
    assert MB.process(sam(refs, recs, header_order=["c3", "c2", "c3", "c1"]), refs, typ="c")[0] == want["c3"] + want["c2"] + want["c1"]


def test_merge_needs_type_cg():
    with pytest.raises(ValueError):
        MB.process(sam({"c1": C1}, [f_read("a", "C", "T")]), {"c1": C1}, typ="c", merge=True)
