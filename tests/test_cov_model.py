"""CPU: tests/cov_model.py (the reference statement of the coverage rule) on hand-made records whose tables are worked out
by hand below: every CIGAR operation, q40 a subset of all, a CpG whose depth is the smaller of its bases', a CpG with one base in a mask, a C
and a G on either side of a contig end and of an N run, overlapping mask intervals, an empty input; the files' text and the uniformity rows."""
import gzip
import cov_model as V

# c1: CpGs at (1,2), (5,6), (10,11), (14,15); ends in C.  c2: starts with G (no CpG across the end); C N G is none; CpG at (4,5)
REFS = {"c1": "ACGTTCGANNCGTTCGC", "c2": "GCnGCG"}


def _rec(flag, chrom, pos, mapq, cigar):
    return "\t".join(["r", str(flag), chrom, str(pos), str(mapq), cigar, "*", "0", "0", "*", "*"])


SAM = "\n".join([
    "@SQ\tSN:c1\tLN:17", "@SQ\tSN:c2\tLN:6",
    _rec(0, "c1", 1, 60, "2S4M1I2M2D3M1H"),      # c1 0-3, 4-5, 8-10             all q40
    _rec(0x110, "c1", 5, 10, "8M"),              # c1 4-11, secondary            all
    _rec(0x400, "c1", 6, 40, "1M"),              # c1 5, duplicate               all q40
    _rec(4, "c1", 1, 0, "*"),                    # unmapped: nothing
    _rec(0x800, "c2", 5, 60, "2M"),              # c2 4-5, supplementary         all q40
    _rec(0, "c2", 6, 3, "1M"),                   # c2 5                          all
]) + "\n"
# depth            0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16
ALL_C1 = [1, 1, 1, 1, 2, 3, 1, 1, 2, 2, 2, 1, 0, 0, 0, 0, 0]
Q40_C1 = [1, 1, 1, 1, 1, 2, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0]
ALL_C2 = [0, 0, 0, 0, 1, 2]
Q40_C2 = [0, 0, 0, 0, 1, 1]
WHOLE = [{0: 9, 1: 8, 2: 5, 3: 1},      # all bases
         {0: 1, 1: 4},                  # all CpGs: min(1,1), min(3,1), min(2,1), 0, min(1,2)
         {0: 12, 1: 10, 2: 1},          # q40 bases
         {0: 3, 1: 2}]                  # q40 CpGs: 1, min(2,0), min(1,0), 0, min(1,1)
TOP = [("c1", 5, 6)]                                        # the C of CpG (5,6) only
BOT = [("c1", 0, 3), ("c1", 2, 7), ("c2", 0, 6)]            # overlapping: c1 0-6 once; all of c2
GC = [{3: 1}, {1: 1}, {2: 1}, {0: 1},
      {0: 4, 1: 6, 2: 2, 3: 1}, {1: 3}, {0: 5, 1: 7, 2: 1}, {0: 1, 1: 2}]


def test_depth_under_m_runs_only_and_q40_is_a_subset():
    dep = V.depths(SAM, REFS)
    assert dep["c1"] == (ALL_C1, Q40_C1) and dep["c2"] == (ALL_C2, Q40_C2)
    assert all(q <= a for c in dep.values() for a, q in zip(*c))


def test_every_cigar_operation():
    sam = _rec(0, "c2", 1, 60, "1H1S1=1X1N1M1I1D1M1S") + "\n"      # = 0, X 1, N skips 2, M 3, I none, D skips 4, M 5
    assert V.depths(sam, REFS)["c2"][0] == [1, 1, 0, 1, 0, 1]
    try:
        V.depths(_rec(0, "c2", 1, 60, "3P") + "\n", REFS)
        assert False
    except ValueError:
        pass


def test_whole_genome_tables_by_hand():
    assert V.tables(SAM, REFS) == WHOLE


def test_gc_tables_by_hand_masked_cpg_and_overlapping_intervals():
    assert V.tables(SAM, REFS, TOP, BOT) == WHOLE + GC
    # the G alone puts the CpG into the mask as well; a mask that touches neither base does not
    assert V.tables(SAM, REFS, [("c1", 6, 7)], [("c1", 7, 10)])[5] == {1: 1} and V.tables(SAM, REFS, [("c1", 6, 7)], [("c1", 7, 10)])[9] == {}


def test_empty_input_has_every_position_at_depth_zero_and_no_uniformity_rows():
    tabs = V.tables("@SQ\tSN:c1\tLN:17\n", REFS, [], [])
    assert tabs[:4] == [{0: 23}, {0: 5}, {0: 23}, {0: 5}] and tabs[4:] == [{}] * 8
    f = V.files(tabs)
    assert f["_cv_table.txt"] == "BISCUITqc Uniformity Table\ngroup\tmu\tsigma\tcv\n"
    assert f["_covdist_all_cpg_table.txt"] == "BISCUITqc Depth Distribution - All CpGs\ndepth\tcount\n0\t5\n"
    assert f["_covdist_q40_base_botgc_table.txt"] == "BISCUITqc Depth Distribution - Q40 Bot GC Bases\ndepth\tcount\n"


def test_files_text_and_uniformity_rows_by_hand():
    f = V.files(V.tables(SAM, REFS, TOP, BOT))
    assert sorted(f) == sorted(V.SUFFIXES) and len(f) == 13
    assert f["_covdist_all_base_table.txt"] == "BISCUITqc Depth Distribution - All Bases\ndepth\tcount\n0\t9\n1\t8\n2\t5\n3\t1\n"
    assert f["_covdist_q40_cpg_topgc_table.txt"] == "BISCUITqc Depth Distribution - Q40 Top GC CpGs\ndepth\tcount\n0\t1\n"
    assert f["_covdist_all_base_botgc_table.txt"] == "BISCUITqc Depth Distribution - All Bot GC Bases\ndepth\tcount\n0\t4\n1\t6\n2\t2\n3\t1\n"
    # mu = sum(c d) / sum(c), sigma^2 = sum(c d^2) / sum(c) - mu^2 worked out by hand; q40_cpg_topgc has sum(c d) = 0: no row
    assert f["_cv_table.txt"] == ("BISCUITqc Uniformity Table\ngroup\tmu\tsigma\tcv\n"
                                  "all_base\t0.913043\t0.880368\t0.964212\n" "all_cpg\t0.8\t0.4\t0.5\n" "q40_base\t0.521739\t0.580072\t1.11181\n"
                                  "q40_cpg\t0.4\t0.489898\t1.22474\n" "all_base_topgc\t3\t0\t0\n" "all_cpg_topgc\t1\t0\t0\n" "q40_base_topgc\t2\t0\t0\n"
                                  "all_base_botgc\t1\t0.877058\t0.877058\n" "all_cpg_botgc\t1\t0\t0\n" "q40_base_botgc\t0.692308\t0.605693\t0.87489\n"
                                  "q40_cpg_botgc\t0.666667\t0.471405\t0.707107\n")
    assert len(V.files(V.tables(SAM, REFS))) == 5


def test_bed_reader_plain_and_gzip(tmp_path):
    text = "# c\ntrack x\nc1\t5\t6\tname\t0.5\n\nc2 0 6\n"
    (tmp_path / "a.bed").write_text(text)
    with gzip.open(str(tmp_path / "a.bed.gz"), "wb") as g:
        g.write(text.encode())
    assert V.read_bed(str(tmp_path / "a.bed")) == V.read_bed(str(tmp_path / "a.bed.gz")) == [("c1", 5, 6), ("c2", 0, 6)]
