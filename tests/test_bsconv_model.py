"""CPU: tests/bsconv_model.py (the independent model of `biscuit bsconv` the product's --bsconv is compared against) on hand-written
records.  Every expected string below was worked out by hand from the rule in the model's docstring:

c1 = GACGTCCATGC   0 G, 1 A, 2 C, 3 G, 4 T, 5 C, 6 C, 7 A, 8 T, 9 G, 10 C     (starts with a G, ends in a C)
c2 = ACNNGTCNACG   0 A, 1 C, 2 N, 3 N, 4 G, 5 T, 6 C, 7 N, 8 A, 9 C, 10 G
c3 = acgtCg        lower case
"""
import bsconv_model as M

REFS = {"c1": "GACGTCCATGC", "c2": "ACNNGTCNACG", "c3": "acgtCg"}


def rec(name, flag, ref, pos, cigar, seq, yd):
    f = [name, str(flag), ref, str(pos), "60", cigar, "*", "0", "0", seq, "I" * len(seq), "NM:i:0"]
    if yd:
        f.append("YD:A:" + yd)
    return f


CASES = [
    # strand f over the whole contig: 2 C>T (next G: CG converted), 5 C>T (next C: CC converted), 6 C kept (next A: CA retained),
    # 10 C kept but it is the last base of the contig: context N, no bucket
    ("f_whole", rec("r", 0, "c1", 1, "11M", "GATGTTCATGC", "f"), "ZN:Z:CA_R1C0,CC_R0C1,CG_R0C1,CT_R0C0"),
    # strand r: 0 G is the first base (context N); 3 G>A, base before is C, complement G: CG converted; 9 G>A, base before T, complement A: CA converted
    ("r_whole", rec("r", 16, "c1", 1, "11M", "GACATCCATAC", "r"), "ZN:Z:CA_R0C1,CC_R0C0,CG_R0C1,CT_R0C0"),
    # an I and a D: M 1-3 (2 C kept, next G: CG retained), I (its C is not counted), M 4-5 (5 C>T, next base is the deleted 6 C: CC converted), D 6, M 7-9
    ("indel", rec("r", 0, "c1", 2, "3M1I2M1D3M", "ACGCTTATG", "f"), "ZN:Z:CA_R0C0,CC_R0C1,CG_R1C0,CT_R0C0"),
    # soft clips advance the read only: M 5-7 = C (kept, next C: CC retained), C>T (next A: CA converted), A
    ("softclip", rec("r", 0, "c1", 6, "2S3M1S", "CCCTAC", "f"), "ZN:Z:CA_R0C1,CC_R1C0,CG_R0C0,CT_R0C0"),
    # hard clips do not advance into SEQ (the deliberate difference from the tool): the same three columns
    ("hardclip", rec("r", 2048, "c1", 6, "2H3M", "CTA", "f"), "ZN:Z:CA_R0C1,CC_R1C0,CG_R0C0,CT_R0C0"),
    # a C at the last base of a contig: context outside the contig
    ("c_at_end", rec("r", 0, "c1", 10, "2M", "GC", "f"), "ZN:Z:CA_R0C0,CC_R0C0,CG_R0C0,CT_R0C0"),
    # a G at the first base
    ("g_at_start", rec("r", 16, "c1", 1, "2M", "GA", "r"), "ZN:Z:CA_R0C0,CC_R0C0,CG_R0C0,CT_R0C0"),
    # context in an N run: 1 C (next N) and 6 C (next N) go nowhere; own base in the run: the read's C over 2 N is skipped; 9 C>T next G: CG converted
    ("n_ctx_f", rec("r", 0, "c2", 1, "11M", "ACCAGTCAATG", "f"), "ZN:Z:CA_R0C0,CC_R0C0,CG_R0C1,CT_R0C0"),
    # ... strand r: 4 G kept, base before is N: nowhere; the read's G over 3 N: skipped; 10 G>A, base before C, complement G: CG converted
    ("n_ctx_r", rec("r", 16, "c2", 1, "11M", "ACAGGTCAACA", "r"), "ZN:Z:CA_R0C0,CC_R0C0,CG_R0C1,CT_R0C0"),
    # YD:u, 2 C>T against 0 G>A: strand 0, as f_whole
    ("u_to_f", rec("r", 0, "c1", 1, "11M", "GATGTTCATGC", "u"), "ZN:Z:CA_R1C0,CC_R0C1,CG_R0C1,CT_R0C0"),
    # YD:u, 0 C>T against 2 G>A: strand 1, as r_whole
    ("u_to_r", rec("r", 0, "c1", 1, "11M", "GACATCCATAC", "u"), "ZN:Z:CA_R0C1,CC_R0C0,CG_R0C1,CT_R0C0"),
    # YD:u, one of each: the tie goes to strand 0: 2 C>T (CG converted), 5 C kept (CC retained), 6 C kept (CA retained)
    ("u_tie", rec("r", 0, "c1", 1, "11M", "GATATCCATGC", "u"), "ZN:Z:CA_R1C0,CC_R1C0,CG_R0C1,CT_R0C0"),
    # lower-case FASTA: 1 c>T next g: CG converted; 4 C kept next g: CG retained
    ("lowercase", rec("r", 0, "c3", 1, "6M", "ATGTCG", "f"), "ZN:Z:CA_R0C0,CC_R0C0,CG_R1C1,CT_R0C0"),
]


def test_hand_written_records():
    conf = M.Conf()
    for name, f, want in CASES:
        keep, zn, retn, conv, filtered = M.record(f, REFS, conf)
        assert keep and not filtered and zn == want, (name, zn, want)


def test_unmapped_passes_unchanged_when_only_annotating():
    f = rec("r", 4, "*", 0, "*", "ACGT", None)
    assert M.record(f, REFS, M.Conf())[:2] == (True, None)


def test_filters_and_totals():
    sam = "\n".join(["@SQ\tSN:c1\tLN:11"] + ["\t".join(f) for _, f, _ in CASES[:4]] + ["\t".join(rec("x", 4, "*", 0, "*", "ACGT", None)), ""])
    # annotate only: five records seen, nothing filtered; totals over f_whole, r_whole, indel, softclip
    out, tot, n, nf = M.process(sam, REFS, M.Conf())
    assert (n, nf) == (5, 0) and tot == [1, 2, 1, 2, 1, 2, 0, 0] and out.count("ZN:Z:") == 4 and out.endswith("\n")
    # at most 0 retained CpA: f_whole (CA_R1) goes, and so does the unmapped record; the kept records all carry ZN
    out, tot, n, nf = M.process(sam, REFS, M.Conf(max_cpa=0))
    assert (n, nf) == (5, 2) and [l.split("\t")[0] for l in out.split("\n") if l and l[0] != "@"] == ["r", "r", "r"] and tot == [0, 2, 1, 1, 1, 1, 0, 0]
    # ... the filtered ones instead: f_whole with its counts, the unmapped record with zeros (the tool appends ZN to whatever it writes)
    out, tot, n, nf = M.process(sam, REFS, M.Conf(max_cpa=0, show_filtered=True))
    kept = [l for l in out.split("\n") if l and l[0] != "@"]
    assert (n, nf) == (5, 2) and len(kept) == 2 and kept[0].endswith("ZN:Z:CA_R1C0,CC_R0C1,CG_R0C1,CT_R0C0") and kept[1].endswith("ZN:Z:CA_R0C0,CC_R0C0,CG_R0C0,CT_R0C0")
    # CpH retention fraction: softclip has 1 retained of 2 CpH = 0.5 > 0.4; f_whole 1 of 2; indel 0 of 1; r_whole 0 of 1
    out, tot, n, nf = M.process(sam, REFS, M.Conf(max_cph_frac=0.4))
    assert (n, nf) == (5, 3)
    # YD:u records go with filter_u
    f = CASES[9][1]
    assert M.record(f, REFS, M.Conf(filter_u=True))[0] is False and M.record(f, REFS, M.Conf(filter_u=True, show_filtered=True))[:2] == (True, "ZN:Z:CA_R0C0,CC_R0C0,CG_R0C0,CT_R0C0")


def test_secondary_without_sequence_takes_it_from_the_primary():
    pri = rec("q", 0, "c1", 1, "11M", "GATGTTCATGC", "f")
    sec = rec("q", 256 | 16, "c1", 6, "5H3M3H", "*", "f")      # reverse strand: the read as printed there is the reverse complement
    by = {("q", 0): [pri, sec]}
    full = M.revcomp("GATGTTCATGC")                              # GCATGAACATC; columns 5-7 take bases 5..7 = A, A, C over C, C, A
    assert full == "GCATGAACATC"
    keep, zn, retn, conv, filtered = M.record(sec, REFS, M.Conf(), by)
    assert zn == "ZN:Z:CA_R0C0,CC_R0C0,CG_R0C0,CT_R0C0"         # read A over both C: neither retained nor converted
