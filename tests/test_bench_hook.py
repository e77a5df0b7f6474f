"""CPU: bench.py's choice of genome: $BISCUIT_HG38_INDEX -> $BISCUIT_HG38_FA -> the synthetic fallback."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_real_genome_source(tmp_path, monkeypatch, capsys):
    b = _bench()
    monkeypatch.delenv("BISCUIT_HG38_INDEX", raising=False)
    monkeypatch.delenv("BISCUIT_HG38_FA", raising=False)
    assert b.real_genome_source() is None
    base = str(tmp_path / "hg38.fa")
    for e in (".par.bwt", ".par.sa", ".dau.bwt", ".dau.sa", ".bis.ann", ".bis.amb"):
        open(base + e, "wb").close()
    monkeypatch.setenv("BISCUIT_HG38_INDEX", base)
    assert b.real_genome_source() is None and ".bis.pac missing" in capsys.readouterr().err      # incomplete: said so, fallback
    open(base + ".bis.pac", "wb").close()
    kind, path, label = b.real_genome_source()
    assert kind == "index" and path == base and base in label
    monkeypatch.delenv("BISCUIT_HG38_INDEX")
    monkeypatch.setenv("BISCUIT_HG38_FA", str(tmp_path / "nope.fa"))
    assert b.real_genome_source() is None and "does not exist" in capsys.readouterr().err
    open(str(tmp_path / "hg38.fa"), "w").write(">c\nACGT\n")
    monkeypatch.setenv("BISCUIT_HG38_FA", str(tmp_path / "hg38.fa"))
    assert b.real_genome_source()[0] == "fasta"
    monkeypatch.setenv("BISCUIT_HG38_INDEX", base)     # the index files win over the FASTA
    assert b.real_genome_source()[0] == "index"


def test_sam_arrays(tmp_path):
    """--dump-outputs: a chunk's SAM text as float64 arrays -- every record of a seeded sample of read pairs, the same sample whatever the
    text, and a summary with the whole text's CRC-32"""
    import re
    import zlib
    import numpy as np
    b = _bench()
    raw = open(os.path.join(ROOT, "tests", "golden", "pe_small.sam"), "rb").read()
    txt = re.sub(rb"(?m)^r(\d{6})\t", lambda m: b"p%09d\t" % int(m.group(1)), raw)     # the bench's read names
    body = [l for l in txt.split(b"\n") if l and not l.startswith(b"@")]
    a = b.sam_arrays(np.frombuffer(txt, dtype=np.uint8), 150, sample=40)
    assert set(a) == {"sam_summary"} | {"sam_" + f for f in b.SAM_FIELDS}
    assert all(v.dtype == np.float64 for v in a.values())
    assert list(a["sam_summary"]) == [len(body), len(txt), zlib.crc32(txt)]
    n = len(a["sam_pair"])
    assert all(len(v) == n for k, v in a.items() if k != "sam_summary") and n >= 80       # 40 pairs, two records each at least
    assert len(set(a["sam_pair"].tolist())) == 40
    rows = [l for l in body if int(l.split(b"\t")[0][1:]) in set(a["sam_pair"].astype(int).tolist())]
    assert [zlib.crc32(l) for l in rows] == a["sam_line_crc32"].astype(np.int64).tolist()        # in output order
    f = rows[0].split(b"\t")
    assert (a["sam_flag"][0], a["sam_pos"][0], a["sam_mapq"][0], a["sam_tlen"][0]) == (int(f[1]), int(f[3]), int(f[4]), int(f[8]))
    assert a["sam_rname_crc32"][0] == zlib.crc32(f[2]) and a["sam_cigar_crc32"][0] == zlib.crc32(f[5])
    assert a["sam_tag_AS"][0] == int([t for t in f[11:] if t.startswith(b"AS:i:")][0][5:])
    # the sample is a property of the arguments, not of the text: a changed record changes its arrays, not which pairs are in them
    p0 = int(a["sam_pair"][0])
    changed = txt.replace(rows[0], rows[0].replace(b"\t60\t", b"\t59\t", 1))
    c = b.sam_arrays(np.frombuffer(changed, dtype=np.uint8), 150, sample=40)
    assert np.array_equal(c["sam_pair"], a["sam_pair"]) and c["sam_mapq"][0] == 59 and p0 == int(c["sam_pair"][0])
    assert c["sam_summary"][2] != a["sam_summary"][2]
    b.write_outputs(str(tmp_path / "out"), a)
    assert np.array_equal(np.load(str(tmp_path / "out" / "sam_pos.npy")), a["sam_pos"])
