"""Shared by tests/test_bam_cpu.py (CPU suite) and tests/test_gpu_bam.py (-m gpu): the data of e2e_cases.make_data at a small size, a `--bam` run
beside the plain run of the same command line, and the comparison of the two through tests/bam_model.py."""
import os
import subprocess
import bam_model as M
import e2e_cases as E

ENV_CLEAR = ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "BSX_OUT", "BSX_GATHER_ID")
# command lines beyond e2e_cases.CASES_CORE whose records hold what the core cases do not: a read group and -I, -p's mixed templates, reads that
# align nowhere or are shorter than a seed, qualities that vary
CASES = E.CASES_CORE + [c for c in E.CASES_MORE if c[0] in ("pe150_fixed_isize_rg", "smart_pairing", "edge_reads", "pe150_clip_qual_adaptor")]
CASES = [(n, [a for a in args if a != "-C"]) for n, args in CASES]      # (a free-text comment is no tag: see the refusals)


def make_data(d):
    return E.make_data(d, 200000, 300, 24, repeat_frac=0.1)


def run_raw(exe, args, d, env=None, timeout=1800):
    e = dict(os.environ)
    for k in ENV_CLEAR:
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([exe] + list(args), cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=e)


def run_pair(exe, opts, args, d, env=None, bam_env=None):
    """the command line without and with --bam -> (SAM bytes, BAM bytes)"""
    p = run_raw(exe, list(opts) + list(args), d, env)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    e = dict(env or {})
    e.update(bam_env or {})
    q = run_raw(exe, ["--bam"] + list(opts) + list(args), d, e)
    assert q.returncode == 0, q.stderr.decode()[-3000:]
    return p.stdout, q.stdout


def split_sam(sam):
    at = 0
    while sam[at:at + 1] == b"@":
        at = sam.index(b"\n", at) + 1
    return sam[:at], sam[at:]


def no_pg(text):
    return b"".join(l + b"\n" for l in text.split(b"\n")[:-1] if not l.startswith(b"@PG"))


def check_bam(bam, sam, what):
    """the file against the model's encoding of `sam` (the @PG line, which holds the command line, aside) -> (payload, header part's length)"""
    sizes = []
    payload = M.bgzf_payload(bam, sizes)                       # every member's framing, CRC and ISIZE; the EOF block byte for byte
    text, refs, recs = M.split_payload(payload)
    hdr, body = split_sam(sam)
    assert no_pg(text) == no_pg(hdr) and text.count(b"@PG") == hdr.count(b"@PG") <= 1, what
    hp = M.encode_header(text)
    assert payload.startswith(hp) and refs == M.header_refs(text), what
    want, bad = M.encode_body(body, M.ref_ids(refs))
    assert bad is None, (what, bad)
    got = payload[len(hp):]
    if got != want:
        at = next(i for i in range(min(len(got), len(want))) if got[i] != want[i])
        raise AssertionError("%s: the record stream differs from the model's at byte %d of %d / %d" % (what, at, len(got), len(want)))
    # the header part ends its block; every block of the record stream but the last holds 0xff00 bytes
    n_h = (len(hp) + M.BGZF_BLOCK - 1) // M.BGZF_BLOCK
    assert sum(sizes[:n_h]) == len(hp), (what, sizes[:n_h + 1])
    data = sizes[n_h:-1]
    assert sizes[-1] == 0 and all(s == M.BGZF_BLOCK for s in data[:-1]) and (not data or 0 < data[-1] <= M.BGZF_BLOCK), (what, data[-3:])
    assert [M.decode_record(r, refs) for r in recs[:50]] == body.split(b"\n")[:-1][:50], what
    return payload, len(hp)
