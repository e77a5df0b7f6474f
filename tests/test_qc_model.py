"""CPU: tests/qc_model.py on hand-written records; every expected number below is worked out by hand from the rule (the docstring of
qc_model.py; src/qc.c, bsstrand.c, cinread.c, bsconv.c of the reference), column by column in the comments."""
import qc_model as Q

#            0123456789ab
C1 = "ACGTCCGATCGA"          # C at 1 (next G), 4 (next C), 5 (next G), 9 (next G); G at 2, 6, 10 (each after a C)
#            01234567890123
C2 = "AGGTCGAGCTGAGG"        # G at 1 (after A), 2 (after G), 5 (after C), 7 (after A), 10, 12, 13
C3 = "TCNNATC"               # C at 1 before an N run, C at 6 as the contig's last base
C5 = "A" * 300 + "CCC" + "A" * 5
REFS = {"c1": C1, "c2": C2, "c3": C3, "c5": C5}


def rec(name, flag, ref, pos, mapq, cigar, tlen, seq, yd):
    return "\t".join([name, str(flag), ref, str(pos), str(mapq), cigar, "=", "1", str(tlen), seq, "*", "NM:i:0", "YD:A:" + yd])


def cells(c):
    """the non-zero read-position cells as {(table, read, position, 'C' or 'R'): count}"""
    out = {}
    for k in range(2):
        for i in range(2):
            for j in range(Q.READ_LEN):
                for s in range(2):
                    if c.readpos[k][i][j][s]:
                        out[("CG" if k == 0 else "CH", i + 1, j, "CR"[s])] = c.readpos[k][i][j][s]
    return out


# forward, read 1, proper pair, TLEN 1000: C1 12M; read T at 1 (converted, CG), C at 4 (retained, next C: CH), T at 5 (converted, CG), C at 9 (retained, CG)
FWD = rec("a", 99, "c1", 1, 60, "12M", 1000, "ATGTCTGATCGA", "f")
# reverse, read 2, proper pair, TLEN 1001, 2S3M1I2M1D3M from POS 2 of C2: columns (ref, qpos): (1,2) (2,3) (3,4) | I at 5 | (4,6) (5,7) | D of 6 | (7,8) (8,9) (9,10)
# YD:r: G columns.  ref 1: read A converted, before it A -> T: CH, position 11 - 2 = 9.  ref 2: read G retained, before it G -> C: CH, 11 - 3 = 8.
# ref 5: read G retained, before it C -> G: CG, 11 - 7 = 4.  ref 7: read A converted, before it A -> T: CH, 11 - 8 = 3.
REV = rec("a", 147, "c2", 2, 60, "2S3M1I2M1D3M", 1001, "TTAGTCCGACT", "r")


def test_forward_read1_and_reverse_read2_with_clip_insertion_deletion():
    c = Q.process(FWD + "\n" + REV + "\n", REFS)
    assert cells(c) == {("CG", 1, 1, "C"): 1, ("CH", 1, 4, "R"): 1, ("CG", 1, 5, "C"): 1, ("CG", 1, 9, "R"): 1,
                        ("CH", 2, 9, "C"): 1, ("CH", 2, 8, "R"): 1, ("CG", 2, 4, "R"): 1, ("CH", 2, 3, "C"): 1}
    # totals: CpA_R CpA_C CpC_R CpC_C CpG_R CpG_C CpT_R CpT_C.  FWD: CpC_R 1, CpG_C 2, CpG_R 1.  REV: CpT_C 2, CpC_R 1, CpG_R 1.
    assert c.conv == [0, 0, 2, 0, 2, 2, 0, 2]
    # FWD: nC2T 2, nG2A 0 -> f under tag f; REV: nG2A 2 (ref 1, 7), nC2T 0 (C columns 4 and 8 read C) -> r under tag r
    assert c.confusion == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert c.strandcnt[0] == 1 and c.strandcnt[8 + 4 + 1] == 1 and sum(c.strandcnt) == 2
    assert c.mapq[60] == 2 and sum(c.mapq) == 2 and (c.all_tot, c.q40_tot, c.all_dup, c.q40_dup) == (2, 2, 0, 0)
    assert c.isize[1000] == 1 and c.n_isize == 1 and sum(c.isize) == 1        # TLEN 1000 counts, 1001 does not
    f = Q.files(c, True)
    assert f["_strand_table.txt"] == ("BISCUITqc Strand Table\nStrand Distribution:\nstrand\\BS      BSW (f)      BSC (r)\n"
                                      "     R1 (f):   1            \n0            \n     R1 (r):   0            \n0            \n"
                                      "     R2 (f):   0            \n0            \n     R2 (r):   0            \n1            \n")
    assert f["_totalReadConversionRate.txt"] == "BISCUITqc Conversion Rate by Read Average Table\nCpA\tCpC\tCpG\tCpT\n-nan\t1.00000000\t0.50000000\t0.00000000\n"
    assert f["_CpGRetentionByReadPos.txt"] == ("BISCUITqc CpG Retention by Read Position Table\nReadInPair\tPosition\tConversion/Retention\tCount\n"
                                               "1\t1\tC\t1\n1\t5\tC\t1\n1\t9\tR\t1\n2\t4\tR\t1\n")
    assert f["_CpHRetentionByReadPos.txt"].endswith("Count\n1\t4\tR\t1\n2\t3\tC\t1\n2\t8\tR\t1\n2\t9\tC\t1\n")
    assert f["_isize_table.txt"] == "BISCUITqc Insert Size Table\nInsertSize\tFraction\tReadCount\n1000\t1.00000000\t1\n"
    assert f["_dup_report.txt"] == ("BISCUITqc Read Duplication Table\nNumber of duplicate reads:\t0\nNumber of reads:\t2\n"
                                    "Number of duplicate q40-reads:\t0\nNumber of q40-reads:\t2\n")
    m = f["_mapq_table.txt"].split("\n")
    assert m[:3] == ["BISCUITqc Mapping Quality Table", "MapQ\tCount", "unmapped\t0"] and m[3] == "0\t0" and m[63] == "60\t2" and len(m) == 65
    assert "_isize_table.txt" not in Q.files(c, False)


def test_hard_clipped_supplementary_counts_positions_of_the_whole_read():
    # read r3 as sequenced: CCCCCTTCGA; a forward supplementary 5H5M at POS 4 of C1: ref 3..7 = TCCGA against TTCGA, whole-read positions 5..9.
    # ref 4: read T converted, next C: CH at position 6.  ref 5: read C retained, next G: CG at position 7.
    fwd = rec("r3", 2048 + 65, "c1", 4, 60, "5H5M", 0, "TTCGA", "f")
    c = Q.process(fwd + "\n", REFS, reads={("r3", 0x40): "CCCCCTTCGA"})
    assert cells(c) == {("CH", 1, 6, "C"): 1, ("CG", 1, 7, "R"): 1} and c.conv == [0] * 8 and c.seen["H"] == 1
    # the same five bases as a reverse record, 5M5H: the whole read as the record has it is TTCGA + AAAAA, so the read as sequenced is its
    # reverse complement; positions are 10 - qpos: ref 4 at qpos 1 -> 9, ref 5 at qpos 2 -> 8
    rev = rec("r4", 2048 + 65 + 16, "c1", 4, 60, "5M5H", 0, "TTCGA", "f")
    c = Q.process(rev + "\n", REFS, reads={("r4", 0x40): Q.revcomp("TTCGAAAAAA")})
    assert cells(c) == {("CH", 1, 9, "C"): 1, ("CG", 1, 8, "R"): 1}
    # without `reads` the whole read comes from the primary record of the same read
    prim = rec("r3", 65, "c2", 1, 0, "10M", 0, "CCCCCTTCGA", "f")
    assert cells(Q.process(prim + "\n" + fwd + "\n", REFS)) == {("CH", 1, 6, "C"): 1, ("CG", 1, 7, "R"): 1}


def test_yd_u_resolved_to_each_strand_and_the_tie():
    # nC2T 1 (ref 1), nG2A 0 -> strand 0, inferred f: C columns 1 (T: converted, CG), 4 (C: retained, CH), 5 (retained, CG), 9 (retained, CG)
    c = Q.process(rec("u0", 0, "c1", 1, 60, "12M", 0, "ATGTCCGATCGA", "u") + "\n", REFS)
    assert cells(c) == {("CG", 1, 1, "C"): 1, ("CH", 1, 4, "R"): 1, ("CG", 1, 5, "R"): 1, ("CG", 1, 9, "R"): 1} and c.confusion[3 * 4 + 0] == 1
    # nG2A 1 (ref 2), nC2T 0 -> strand 1, inferred r: G columns 2 (A: converted), 6, 10 (retained); each follows a C: all CG
    c = Q.process(rec("u1", 0, "c1", 1, 60, "12M", 0, "ACATCCGATCGA", "u") + "\n", REFS)
    assert cells(c) == {("CG", 1, 2, "C"): 1, ("CG", 1, 6, "R"): 1, ("CG", 1, 10, "R"): 1} and c.confusion[3 * 4 + 1] == 1
    # the tie 1 : 1 -> inferred conflict (min / max = 1), and infer_bsstrand says strand 0 (nC2T >= nG2A)
    c = Q.process(rec("u2", 0, "c1", 1, 60, "12M", 0, "ATATCCGATCGA", "u") + "\n", REFS)
    assert cells(c) == {("CG", 1, 1, "C"): 1, ("CH", 1, 4, "R"): 1, ("CG", 1, 5, "R"): 1, ("CG", 1, 9, "R"): 1} and c.confusion[3 * 4 + 2] == 1
    # nothing converted -> inferred unknown, strand 0, every C retained
    c = Q.process(rec("u3", 0, "c1", 1, 60, "12M", 0, C1, "u") + "\n", REFS)
    assert cells(c) == {("CG", 1, 1, "R"): 1, ("CH", 1, 4, "R"): 1, ("CG", 1, 5, "R"): 1, ("CG", 1, 9, "R"): 1} and c.confusion[3 * 4 + 3] == 1
    # single-end records have no 0x40: the strand table files them under R2 (bsstrand.c:154), forward, tag u = column 3 (not printed)
    assert c.strandcnt[8 + 3] == 1 and c.seen["yd_u"] == 1


def test_the_four_inferred_classes_and_the_integer_division():
    def inferred(seq, yd="f"):
        c = Q.process(rec("x", 0, "c1", 1, 39, "12M", 0, seq, yd) + "\n", REFS)
        assert cells(c) == {} and c.q40_tot == 0          # MAPQ 39: no read-position counts
        (k,) = [i for i, v in enumerate(c.confusion) if v]
        assert k // 4 == Q.TAGS[yd]
        return k % 4
    assert inferred("ATGTCCGATCGA") == 0                   # 1 : 0 -> f
    assert inferred("ACATCCGATCGA", "r") == 1              # 0 : 1 -> r
    assert inferred("ATATCCGATCGA") == 2                   # 1 : 1 -> conflict
    assert inferred(C1) == 3                               # 0 : 0 -> unknown
    assert inferred("ATATCTGATCGA") == 0                   # nC2T 2 (ref 1, 5), nG2A 1 (ref 2): ratio exactly 0.5 -> f
    assert inferred("ACATCCAATCGA", "r") == 1              # nG2A 2 (ref 2, 6), nC2T 0 -> r
    assert inferred("ATATCCAATCGA", "r") == 1              # nC2T 1, nG2A 2: exactly 0.5 -> r
    assert inferred("ATATTTAATCGA") == 0                   # nC2T 3 (ref 1, 4, 5), nG2A 2 (ref 2, 6): 2 / 3 is 0 as integers -> f, not conflict
    assert Q.infer(3, 2) == 0 and Q.infer(2, 3) == 1 and Q.infer(5, 5) == 2


def test_neighbour_in_an_n_run_and_at_the_contig_end():
    # C3 = TCNNATC, 7M, YD:f, proper pair with TLEN 0.  ref 1: read C retained, next is N: CH, no conversion total.  ref 2, 3: N columns, skipped
    # (the read's A there is nothing).  ref 6: read T converted, next is beyond the contig: CH, no total.
    c = Q.process(rec("n", 99, "c3", 1, 60, "7M", 0, "TCAAATT", "f") + "\n", REFS)
    assert cells(c) == {("CH", 1, 1, "R"): 1, ("CH", 1, 6, "C"): 1} and c.conv == [0] * 8
    assert c.confusion[0] == 1 and c.isize[0] == 1
    # the same on the other strand: G as a contig's first base has nothing before it
    c = Q.process(rec("n2", 0, "g", 1, 60, "3M", 0, "AAC", "r") + "\n", {"g": "GAC"})
    assert cells(c) == {("CH", 1, 0, "C"): 1}


def test_mapq_39_and_40_secondary_unmapped():
    lines = [rec("p", 0, "c1", 1, 39, "12M", 0, "ATGTCCGATCGA", "f"), rec("q", 0, "c1", 1, 40, "12M", 0, "ATGTCCGATCGA", "f"),
             rec("q", 256, "c1", 1, 60, "12M", 0, "*", "f"),       # secondary, printed without SEQ: the read comes from q's primary record
             "\t".join(["z", "4", "*", "0", "0", "*", "*", "0", "0", "ACGT", "*", "YD:A:u"])]
    c = Q.process("@HD\tVN:1.5\n" + "\n".join(lines) + "\n", REFS)
    assert (c.all_tot, c.q40_tot) == (4, 2)                # the secondary's MAPQ 60 counts among the q40 reads
    assert c.mapq[39] == 1 and c.mapq[40] == 1 and c.mapq[Q.N_MAPQ] == 1 and sum(c.mapq) == 3      # ... but not in the histogram
    assert cells(c) == {("CG", 1, 1, "C"): 1, ("CH", 1, 4, "R"): 1, ("CG", 1, 5, "R"): 1, ("CG", 1, 9, "R"): 1}      # q's primary only
    assert c.confusion[0] == 3 and c.strandcnt[8] == 3     # bsstrand looks at all three mapped records
    assert c.seen["below40"] == 1 and c.seen["q40"] == 2 and c.seen["secondary"] == 1


def test_tlen_bounds_need_a_proper_pair():
    mk = lambda flag, mapq, tlen: rec("t", flag, "c1", 1, mapq, "12M", tlen, C1, "f")
    c = Q.process("\n".join([mk(99, 60, 1000), mk(99, 60, 1001), mk(99, 60, 0), mk(99, 60, -5), mk(97, 60, 300), mk(99, 39, 300), mk(99 + 256, 60, 300)]), REFS)
    assert c.isize[1000] == 1 and c.isize[0] == 1 and sum(c.isize) == 2 and c.n_isize == 2


def test_positions_300_301_302():
    # C5: C at 300, 301, 302 (next C, C, A: all CH); a forward read of 308 bases retains all three: only position 300 is counted
    c = Q.process(rec("l", 0, "c5", 1, 60, "308M", 0, C5, "f") + "\n", REFS)
    assert cells(c) == {("CH", 1, 300, "R"): 1} and c.seen["pos_gt150"] == 1
    # as a reverse record the positions are 308 - qpos: 8, 7, 6
    c = Q.process(rec("l", 16, "c5", 1, 60, "308M", 0, C5, "f") + "\n", REFS)
    assert cells(c) == {("CH", 1, 8, "R"): 1, ("CH", 1, 7, "R"): 1, ("CH", 1, 6, "R"): 1}
    # 301 leading soft-clipped bases push a forward record's first column past the table
    c = Q.process(rec("l", 0, "c1", 1, 60, "301S12M", 0, "A" * 301 + C1, "f") + "\n", REFS)
    assert cells(c) == {} and c.confusion[3] == 1
    c = Q.process(rec("l", 0, "c1", 1, 60, "299S12M", 0, "A" * 299 + C1, "f") + "\n", REFS)
    assert cells(c) == {("CG", 1, 300, "R"): 1}           # the C at ref 1 sits at position 300; 303, 304, 308 are dropped
