"""CPU: tests/sort_model.py, the reference statement of `--sort`, on hand-written SAM: what the key is, what a tie is, what happens to the header."""
import sort_model as S


def rec(name, flag, rname, pos, rest="60\t4M\t*\t0\t0\tACGT\tIIII"):
    return "%s\t%d\t%s\t%d\t%s" % (name, flag, rname, pos, rest)


HDR = ["@SQ\tSN:chr10\tLN:1000", "@SQ\tSN:chr2\tLN:1000", "@SQ\tSN:chrM\tLN:100", "@PG\tID:x"]      # (name order, as the aligner writes by default)


def test_rank_is_the_index_among_the_sq_lines_not_the_name_or_the_contig_index():
    body = [rec("a", 0, "chr2", 5), rec("b", 0, "chr10", 900), rec("c", 0, "chrM", 1), rec("d", 0, "chr2", 4)]
    out = S.process("\n".join(HDR + body) + "\n").split("\n")
    assert out[0] == "@HD\tVN:1.6\tSO:coordinate" and out[1:5] == HDR
    assert [l.split("\t")[0] for l in out[5:9]] == ["b", "d", "a", "c"] and out[9] == ""
    assert S.ranks(HDR) == {"chr10": 0, "chr2": 1, "chrM": 2}


def test_a_users_sq_order_decides_and_an_hd_line_in_the_middle_moves_to_the_front():
    hdr = ["@SQ\tSN:chrM\tLN:100", "@CO\tx", "@HD\tVN:1.5\tSO:unsorted\tGO:none", "@SQ\tSN:chr2\tLN:1000", "@SQ\tSN:chr10\tLN:1000"]
    body = [rec("a", 0, "chr10", 1), rec("b", 0, "chr2", 900), rec("c", 16, "chrM", 50)]
    out = S.process("\n".join(hdr + body) + "\n").split("\n")
    assert out[0] == "@HD\tVN:1.5\tSO:coordinate\tGO:none"
    assert out[1:5] == [hdr[0], hdr[1], hdr[3], hdr[4]]
    assert [l.split("\t")[0] for l in out[5:8]] == ["c", "b", "a"]
    assert S.header(["@HD\tVN:1.6", "@SQ\tSN:a\tLN:1"]) == ["@HD\tVN:1.6\tSO:coordinate", "@SQ\tSN:a\tLN:1"]      # no SO: appended
    assert S.header(["@HD"]) == ["@HD\tSO:coordinate"]


def test_star_ranks_last_and_an_unmapped_record_with_its_mates_position_sorts_there():
    body = [rec("u", 77, "*", 0), rec("m2", 133, "chr2", 40), rec("m1", 73, "chr2", 40), rec("x", 0, "chrM", 99), rec("v", 141, "*", 0),
            rec("e", 0, "chr2", 39)]
    out = [l.split("\t")[0] for l in S.split(S.process("\n".join(HDR + body) + "\n"))[1]]
    assert out == ["e", "m2", "m1", "x", "u", "v"]      # the fields decide, not 0x4; the two at chr2:40 forward keep their order
    assert S.key(body[0], S.ranks(HDR)) == (S.NO_RANK, 0, 0) and S.key(rec("z", 0, "nowhere", 3), S.ranks(HDR))[0] == S.NO_RANK


def test_forward_before_reverse_at_one_position_and_ties_keep_the_input_order():
    body = [rec("r1", 16, "chr2", 7), rec("f1", 0, "chr2", 7), rec("r2", 0x10 | 0x100, "chr2", 7), rec("f2", 0x400, "chr2", 7), rec("f3", 99, "chr2", 7),
            rec("r3", 147, "chr2", 7), rec("p", 16, "chr2", 6)]
    out = [l.split("\t")[0] for l in S.split(S.process("\n".join(HDR + body) + "\n"))[1]]
    assert out == ["p", "f1", "f2", "f3", "r1", "r2", "r3"]


def test_nothing_inside_a_line_changes_and_every_line_stays():
    body = [rec("a", 16, "chr2", 5, "0\t*\t=\t5\t0\tAC\t!!\tXA:Z:chr10,+1,2M,0;\tZN:Z:CA_R0C0"), rec("b", 0, "chr10", 5, "7\t2M\tchr2\t5\t-3\tAC\tII")]
    text = "\n".join(HDR + body) + "\n"
    out = S.process(text)
    assert sorted(out.split("\n")[1:]) == sorted(text.split("\n")) and out.endswith(body[0] + "\n")
    assert S.process("\n".join(HDR) + "\n") == "@HD\tVN:1.6\tSO:coordinate\n" + "\n".join(HDR) + "\n"      # no records
