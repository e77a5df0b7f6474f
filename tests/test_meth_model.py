"""CPU: tests/meth_model.py, the reference statement of --qc-meth's rule, on hand-written records over a tiny FASTA -- one or more per clause of
DESIGN.md section 7 -- with every expectation worked out by hand, and its beta in thousandths against '%1.3f' for every 0 <= r <= n <= 1200."""
import meth_model as M

#        0         1         2         3         4         5
#        0123456789012345678901234567890123456789012345678901
C1 = "TTATTCGTTATTCATTATTGATTATTCCTTATTCTTTATTCNGTTATTACGC"
REFS = {"c1": C1, "c2": "GTTATTAC"}
READ = C1.replace("N", "A")
# C at 5 (CG), 12 (CA), 26 (CC), 27 (CT), 33 (CT), 40 (CN: before the N), 49 (CG), 51 (CN: the contig's last base); G at 6 (CG), 19 (CA), 42 (CN:
# behind the N), 50 (CG).  A read over all of c1 has len 52: q1 <= 3 drops 0..2, len < q1 + 3 drops 49..51.
KEPT_C, KEPT_G = [5, 12, 26, 27, 33, 40], [6, 19, 42]


def rec(flag=0, pos=1, mapq=60, cigar="52M", seq=READ, qual=None, yd="f", as_=100, extra=(), rname="c1", pnext=0):
    tags = (["AS:i:%d" % as_] if as_ is not None else []) + (["YD:A:" + yd] if yd else []) + list(extra)
    return "\t".join(["r", str(flag), rname, str(pos), str(mapq), cigar, "=" if pnext else "*", str(pnext), "0", seq, "I" * len(seq) if qual is None else qual] + tags)


def put(seq, **at):
    s = list(seq)
    for k, v in at.items():
        s[int(k[1:])] = v
    return "".join(s)


def nonzero(sam, refs=REFS):
    cnt, seen = M.counts(sam + "\n", refs)
    return {(name, i): tuple(c) for name in cnt for i, c in enumerate(cnt[name]) if any(c)}, seen


def want(ret=(), conv=(), opp_ref=(), opp_alt=(), name="c1"):
    out = {}
    for k, idx in enumerate((ret, conv, opp_ref, opp_alt)):
        for i in idx:
            c = list(out.get((name, i), (0, 0, 0, 0)))
            c[k] += 1
            out[(name, i)] = tuple(c)
    return out


def test_a_forward_read_over_the_contig_both_end_rules_and_the_hole():
    got, seen = nonzero("@SQ\tSN:c1\tLN:52\n" + rec())
    assert got == want(ret=KEPT_C, opp_ref=KEPT_G)
    assert seen["counted"] == 1 and seen["end5"] == 3 and seen["end3"] == 3 and seen["hole"] == 1 and seen["lowq"] == 0 and seen["overlap"] == 0
    got, _ = nonzero(rec(seq=put(READ, p5="T", p12="T", p6="A", p41="C")))      # conversions; A over a G on strand 0; a C over the N counts nowhere
    assert got == want(ret=[26, 27, 33, 40], conv=[5, 12], opp_ref=[19, 42], opp_alt=[6])
    got, _ = nonzero(rec(seq=put(READ, p5="A", p19="T")))                       # other bases count nowhere
    assert got == want(ret=[12, 26, 27, 33, 40], opp_ref=[6, 42])


def test_the_other_strand_and_a_reverse_record():
    got, _ = nonzero(rec(yd="r", seq=put(READ, p19="A", p5="T")))
    assert got == want(ret=[6, 42], conv=[19], opp_ref=[12, 26, 27, 33, 40], opp_alt=[5])
    got, seen = nonzero(rec(flag=16))                                          # the record is not turned round: q1 counts along SEQ as printed
    assert got == want(ret=KEPT_C, opp_ref=KEPT_G) and seen["reverse"] == 1
    got, _ = nonzero(rec(flag=16, pos=3, cigar="50M", seq=READ[2:]))            # len 50: q1 <= 3 drops 2..4, len < q1 + 3 drops 49..51
    assert got == want(ret=KEPT_C, opp_ref=KEPT_G)
    got, _ = nonzero(rec(flag=16, pos=4, cigar="46M", seq=READ[3:49]))          # 3..48: drops 3..5 and 46..48
    assert got == want(ret=[12, 26, 27, 33, 40], opp_ref=KEPT_G)


def test_each_record_filter():
    base = want(ret=KEPT_C, opp_ref=KEPT_G)
    for why, kw in (("unmapped", dict(flag=4)), ("secondary", dict(flag=0x100)), ("qcfail", dict(flag=0x200)), ("dup", dict(flag=0x400)), ("mapq", dict(mapq=39)),
                    ("short", dict(cigar="9M", seq=READ[:9])), ("improper", dict(flag=0x1 | 0x40)), ("as", dict(as_=39))):
        got, seen = nonzero(rec(**kw))
        assert got == {} and seen[why] == 1 and seen["counted"] == 0, why
    for kw in (dict(mapq=40), dict(flag=0x1 | 0x2 | 0x40), dict(as_=40), dict(as_=None), dict(flag=0x800)):
        got, seen = nonzero(rec(**kw))
        assert got == base and seen["counted"] == 1, kw
    got, seen = nonzero(rec(pos=3, cigar="10M", seq=READ[2:12]))               # ten bases count: 2..11, q1 4..7 are 5..8
    assert got == want(ret=[5], opp_ref=[6]) and seen["counted"] == 1
    got, seen = nonzero(rec(flag=0x100, seq="*", qual="*"))
    assert got == {} and seen["secondary"] == 1


def test_quality_floor_on_columns_and_no_qualities():
    q = list("I" * 52)
    q[5], q[12], q[26] = "#", "4", "5"                                          # 2, 19, 20
    got, seen = nonzero(rec(qual="".join(q)))
    assert got == want(ret=[26, 27, 33, 40], opp_ref=KEPT_G) and seen["lowq"] == 2
    got, seen = nonzero(rec(qual="*"))
    assert got == want(ret=KEPT_C, opp_ref=KEPT_G) and seen["lowq"] == 0


def test_an_inferred_strand_uses_the_quality_floor():
    seq = put(READ, p5="T", p6="A", p19="A")
    q = list("I" * 52)
    q[6] = q[19] = "+"                                                          # 10: at quality 0 nG2A = 2 > nC2T = 1, at quality 20 nG2A = 0
    got, seen = nonzero(rec(yd="u", seq=seq, qual="".join(q)))
    assert got == want(ret=[12, 26, 27, 33, 40], conv=[5], opp_ref=[42]) and seen["inferred"] == 1
    got, _ = nonzero(rec(yd="u", seq=seq))                                      # all high: nG2A = 2 > nC2T = 1 -> strand 1
    assert got == want(ret=[42], conv=[6, 19], opp_ref=[12, 26, 27, 33, 40], opp_alt=[5])
    got, _ = nonzero(rec(yd="u", seq=put(READ, p5="T", p6="A")))                # a tie -> strand 0
    assert got == want(ret=[12, 26, 27, 33, 40], conv=[5], opp_ref=[19, 42], opp_alt=[6])
    got, _ = nonzero(rec(yd=None, seq=seq))                                     # no YD at all: inferred as well
    assert got == want(ret=[42], conv=[6, 19], opp_ref=[12, 26, 27, 33, 40], opp_alt=[5])
    got, _ = nonzero(rec(yd="u", seq=put(READ, p50="A")))                       # the inference looks at the columns the end rules drop: nG2A = 1 > 0
    assert got == want(ret=KEPT_G, opp_ref=KEPT_C)


def test_hard_and_soft_clips_count_towards_q1_and_len():
    got, seen = nonzero(rec(pos=6, cigar="2H3S40M", seq="GGG" + READ[5:45]))    # len 45, first column q1 = 6; q1 > 42 drops 42..44
    assert got == want(ret=KEPT_C, opp_ref=[6, 19]) and seen["H"] == 1 and seen["S"] == 1
    got, _ = nonzero(rec(cigar="40M3S2H", seq=READ[:40] + "CCC"))               # len 45: 0..2 dropped, nothing at the far end
    assert got == want(ret=[5, 12, 26, 27, 33], opp_ref=[6, 19])
    got, _ = nonzero(rec(pos=6, cigar="1H40M", seq=READ[5:45]))                 # q1 of positions 5, 6 is 2, 3: dropped; len 41: q1 > 38 drops 42..44
    assert got == want(ret=[12, 26, 27, 33, 40], opp_ref=[19])
    q = "I" * 3 + "#" + "I" * 39                                                # QUAL is indexed as SEQ is: the low base is position 5
    got, _ = nonzero(rec(pos=6, cigar="2H3S40M", seq="GGG" + READ[5:45], qual=q))
    assert got == want(ret=[12, 26, 27, 33, 40], opp_ref=[6, 19])


def test_insertions_and_deletions():
    got, seen = nonzero(rec(cigar="10M2I10M3D20M", seq=READ[:10] + "CC" + READ[10:20] + READ[23:43]))      # len 42: q1 > 39 drops 40..42
    assert got == want(ret=[5, 12, 26, 27, 33], opp_ref=[6, 19]) and seen["I"] == 1 and seen["D"] == 1
    got, _ = nonzero(rec(cigar="5M1D46M", seq=READ[:5] + READ[6:]))             # the C at 5 deleted; len 51 drops 49..51 all the same
    assert got == want(ret=[12, 26, 27, 33, 40], opp_ref=KEPT_G)


def test_read_2_leaves_the_overlap_to_its_mate():
    r2, r1 = 0x1 | 0x2 | 0x80, 0x1 | 0x2 | 0x40
    got, seen = nonzero(rec(flag=r2, pnext=21, extra=["MC:Z:20M"]))             # the mate covers 21..40 (1-based): 20..39 dropped
    assert got == want(ret=[5, 12, 40], opp_ref=KEPT_G) and seen["overlap"] == 20
    got, _ = nonzero(rec(flag=r2, pnext=21, extra=["MC:Z:5S10M2D8M3I"]))        # reference length 20 again
    assert got == want(ret=[5, 12, 40], opp_ref=KEPT_G)
    got, seen = nonzero(rec(flag=r2, pnext=21, extra=["MC:Z:*"]))
    assert got == want(ret=KEPT_C, opp_ref=KEPT_G) and seen["overlap"] == 0
    got, _ = nonzero(rec(flag=r1, pnext=21, extra=["MC:Z:20M"]))                # read 1 keeps its columns
    assert got == want(ret=KEPT_C, opp_ref=KEPT_G)
    got, _ = nonzero(rec(flag=r2, pnext=21))                                    # no MC: the mate is taken to be as long as the record
    assert got == want(ret=[5, 12], opp_ref=[6, 19])
    got, _ = nonzero(rec(flag=r2, pos=21, cigar="32M", seq=READ[20:], pnext=1, extra=["MC:Z:30M"]))      # the mate starts first: 21..30 -> 20..29
    assert got == want(ret=[33, 40], opp_ref=[42])                              # (20..22 fall to q1 <= 3 as well, 49..51 to the far end)


def _cnt(**sites):
    cnt = {name: [[0, 0, 0, 0] for _ in seq] for name, seq in REFS.items()}
    for k, v in sites.items():
        name, i = k.split("_")
        cnt[name][int(i)] = list(v)
    return cnt


def test_contexts_holes_and_contig_ends():
    assert [M.context(C1, i) for i in (5, 12, 26, 27, 33, 49)] == [2, 0, 1, 3, 3, 2]
    assert [M.context(C1, i) for i in (6, 19, 50)] == [2, 0, 2]                 # the complement of the base before: C -> G, T -> A
    assert [M.context(C1, i) for i in (40, 42, 51)] == [4, 4, 4]                # the N as a neighbour; the contig's last base
    assert M.context(REFS["c2"], 0) == 4 and M.context(REFS["c2"], 7) == 4      # G as a contig's first base, C as its last
    K, S, unc = M.tables(_cnt(c1_5=(1, 0, 0, 0), c1_6=(0, 1, 0, 0), c1_12=(1, 1, 0, 0), c1_40=(1, 0, 0, 0), c1_42=(1, 0, 0, 0), c1_51=(1, 0, 0, 0),
                              c2_0=(1, 0, 0, 0), c2_7=(0, 3, 0, 0), c1_41=(5, 0, 0, 0), c1_0=(5, 0, 0, 0)), REFS)
    assert K == [1, 0, 2, 0, 5] and S == [500, 0, 1000, 0, 4000] and unc == 0   # counters at the N and at a T are no site


def test_callability_and_its_boundary():
    for c, ok in (((19, 1, 1, 1), False), ((20, 1, 1, 1), True), ((10, 0, 11, 1), True), ((10, 0, 10, 1), False), ((0, 5, 0, 1), False), ((40, 0, 1, 2), True),
                  ((39, 1, 1, 2), False), ((7, 3, 9, 0), True)):
        K, S, unc = M.tables(_cnt(c1_5=c), REFS)
        assert (K[2], unc) == ((1, 0) if ok else (0, 1)), c
        assert M.callable_site(*c) == ok
    K, S, unc = M.tables(_cnt(c1_5=(0, 0, 4, 1)), REFS)                         # ret + conv == 0: not a site at all
    assert K == [0] * 5 and unc == 0


def test_fewer_than_twenty_sites_print_minus_one():
    assert M.file_text([19, 20, 0, 40, 99], [19000, 12345, 0, 1, 5]) == M.TITLE + "CA\tCC\tCG\tCT\n-1\t0.61725\t-1\t2.5e-05\n"
    assert M.file_text([20, 20, 20, 3000000], [20000, 0, 6667, 1234567891]) == M.TITLE + "CA\tCC\tCG\tCT\n1\t0\t0.33335\t0.411523\n"
    assert M.process("", REFS)[0] == M.TITLE + "CA\tCC\tCG\tCT\n-1\t-1\t-1\t-1\n"


def test_milli_equals_printf_for_every_pair_up_to_1200():
    ties = 0
    for n in range(1, 1201):
        for r in range(n + 1):
            m = M.milli(r, n)
            assert "%d.%03d" % divmod(m, 1000) == "%1.3f" % (r / n), (r, n, m)
            if 2 * (1000 * r % n) == n:
                ties += 1
    assert ties == 1560
    assert M.milli(1, 16) == 62 and M.milli(3, 16) == 188                       # exact ties: 0.0625 -> 0.062, 0.1875 -> 0.188 (to even)
    assert (M.milli(1, 80), M.milli(3, 80), M.milli(7, 80)) == (13, 37, 87)     # inexact ties: the doubles lie above 0.0125, below 0.0375 and below 0.0875
    assert (M.milli(1, 3), M.milli(2, 3), M.milli(0, 7), M.milli(7, 7)) == (333, 667, 0, 1000)
