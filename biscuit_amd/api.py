"""Thin Python mirror of the C ABI (include/bsx.h) over numpy buffers -- test/bench plumbing."""
import ctypes as C
import numpy as np
from . import _lib as B

SORT_TILE = B.SORT_TILE      # BSX_SORT_TILE (include/bsx.h): the sizes around it are where Device.sort_run changes kernels

SEED_DT = np.dtype(B.SeedTask)
SA_DT = np.dtype(B.SaJob)
EXT_DT = np.dtype(B.ExtJob)
EXTRES_DT = np.dtype(B.ExtRes)
SW_DT = np.dtype(B.SwJob)
SWRES_DT = np.dtype(B.SwRes)
GLB_DT = np.dtype(B.GlbJob)
GLBRES_DT = np.dtype(B.GlbRes)
INTV_DT = np.dtype(B.Intv)


def default_opt():
    o = B.Opt()
    B.lib().bsx_opt_init(C.byref(o))
    return o


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Index:
    """<base>.{par,dau}.{bwt,sa} + <base>.bis.{ann,amb,pac} (bwa_idx_load_from_disk, lib/aln/bwa.c:525)"""

    def __init__(self, base):
        self.base = base
        self.h = C.c_void_p()
        B.check(B.lib().bsx_index_load(base.encode(), C.byref(self.h)), "bsx_index_load(%s)" % base)
        self.l_pac = B.lib().bsx_index_l_pac(self.h)

    @staticmethod
    def build(fasta, base):
        B.check(B.lib().bsx_index_build(fasta.encode(), base.encode()), "bsx_index_build")
        return Index(base)

    @classmethod
    def _wrap(cls, h):
        self = cls.__new__(cls)
        self.base = None
        self.h = h
        self.l_pac = B.lib().bsx_index_l_pac(h)
        return self

    @classmethod
    def from_fasta(cls, fasta):
        """pac + annotation only (bis_bns_fasta2bntseq); the FM indices come from build_host() or Device.build_index()"""
        h = C.c_void_p()
        B.check(B.lib().bsx_index_from_fasta(fasta.encode(), C.byref(h)), "bsx_index_from_fasta")
        return cls._wrap(h)

    @classmethod
    def synthetic(cls, n_bases, seed, n_contigs=8, repeat_frac=0.05, profile=0):
        """seeded synthetic genome (csrc/host/sim.c) straight into an index without FM indices; profile 1 = with the high-copy
        interspersed repeat families of a mammalian genome (~43 % repeats)"""
        L = B.lib()
        L.bsx_sim_genome_index2.argtypes = [C.c_int64, C.c_uint64, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_void_p)]
        h = C.c_void_p()
        B.check(L.bsx_sim_genome_index2(n_bases, seed, n_contigs, repeat_frac, profile, C.byref(h)), "bsx_sim_genome_index2")
        return cls._wrap(h)

    def build_host(self):
        B.check(B.lib().bsx_index_build_host(self.h), "bsx_index_build_host")

    def save(self, base):
        B.check(B.lib().bsx_index_save(self.h, base.encode()), "bsx_index_save")

    def close(self):
        if self.h:
            B.lib().bsx_index_free(self.h)
            self.h = None


class Batches:
    """The five kernel-level batch seams, bound either to the HIP device or (tests only) to the
    CPU restatement in oracle/."""

    def __init__(self, fns, ctx):
        self.f = fns
        self.ctx = ctx
        self._keep = None

    def set_opt(self, opt):
        B.check(self.f["set_opt"](self.ctx, C.byref(opt)), "set_opt")

    def set_reads(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        self._keep = buf
        B.check(self.f["set_reads"](self.ctx, _p(buf), C.c_size_t(buf.size)), "set_reads")

    def seed(self, opt, tasks):
        tasks = np.ascontiguousarray(tasks, dtype=SEED_DT)
        n = len(tasks)
        out = C.c_void_p()
        cap = C.c_int64(0)
        off = np.zeros(n + 1, dtype=np.int64)
        B.check(self.f["seed_batch"](self.ctx, C.byref(opt), C.c_int64(n), _p(tasks), C.byref(out), C.byref(cap), _p(off)), "seed_batch")
        tot = int(off[n])
        if tot:
            arr = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(tot, 4)).copy()
        else:
            arr = np.zeros((0, 4), dtype=np.uint64)
        if out.value:
            _libc_free(out)
        return arr, off

    def sa(self, jobs):
        jobs = np.ascontiguousarray(jobs, dtype=SA_DT)
        pos = np.zeros(len(jobs), dtype=np.uint64)
        B.check(self.f["sa_batch"](self.ctx, C.c_int64(len(jobs)), _p(jobs), _p(pos)), "sa_batch")
        return pos

    def extend(self, jobs):
        jobs = np.ascontiguousarray(jobs, dtype=EXT_DT)
        res = np.zeros(len(jobs), dtype=EXTRES_DT)
        B.check(self.f["extend_batch"](self.ctx, C.c_int64(len(jobs)), _p(jobs), _p(res)), "extend_batch")
        return res

    def sw(self, jobs):
        jobs = np.ascontiguousarray(jobs, dtype=SW_DT)
        res = np.zeros(len(jobs), dtype=SWRES_DT)
        B.check(self.f["sw_batch"](self.ctx, C.c_int64(len(jobs)), _p(jobs), _p(res)), "sw_batch")
        return res

    def global_(self, jobs, pool_len):
        jobs = np.ascontiguousarray(jobs, dtype=GLB_DT)
        res = np.zeros(len(jobs), dtype=GLBRES_DT)
        pool = np.zeros(max(1, pool_len), dtype=np.uint32)
        B.check(self.f["global_batch"](self.ctx, C.c_int64(len(jobs)), _p(jobs), _p(res), _p(pool), C.c_size_t(pool.size)), "global_batch")
        return res, pool


_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]


def _libc_free(p):
    _libc.free(p)


def bam_encode(handle, header, text):
    """bsx_bam_encode: handle None = the host's own statement of the record rule (csrc/host/bam_rec.h, the source the device compiles)"""
    L = B.lib()
    refs = C.c_void_p()
    L.bsx_bam_refs_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.bsx_bam_refs_close.argtypes = [C.c_void_p]
    B.check(L.bsx_bam_refs_open(bytes(header), C.byref(refs)), "bsx_bam_refs_open")
    out, cap, n, nrec, bad, why = C.c_void_p(), C.c_size_t(0), C.c_size_t(0), C.c_int64(0), C.c_int64(0), C.c_int(0)
    f = L.bsx_bam_encode
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                  C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    try:
        B.check(f(handle, refs, bytes(text), len(text), C.byref(out), C.byref(cap), C.byref(n), C.byref(nrec), C.byref(bad), C.byref(why)), "bsx_bam_encode")
        return (C.string_at(out, n.value) if n.value else b""), bad.value, why.value
    finally:
        if out.value:
            _libc_free(out)
        L.bsx_bam_refs_close(refs)


def bam_header(header):
    """bsx_bam_header: the header part of the BAM payload for the header text (bytes)"""
    L = B.lib()
    out, n = C.c_void_p(), C.c_size_t(0)
    L.bsx_bam_header.argtypes = [C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    B.check(L.bsx_bam_header(bytes(header), C.byref(out), C.byref(n)), "bsx_bam_header")
    try:
        return C.string_at(out, n.value)
    finally:
        _libc_free(out)


def bgzf_deflate(handle, payload):
    """bsx_bgzf_deflate: handle None = the host's statement (zlib level 1 raw, stored when that is no smaller)"""
    L = B.lib()
    out, cap, n = C.c_void_p(), C.c_size_t(0), C.c_size_t(0)
    f = L.bsx_bgzf_deflate
    f.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    try:
        B.check(f(handle, bytes(payload), len(payload), C.byref(out), C.byref(cap), C.byref(n)), "bsx_bgzf_deflate")
        return C.string_at(out, n.value) if n.value else b""
    finally:
        if out.value:
            _libc_free(out)


def cov_tables_arrays(t):
    """a filled _lib.CovTables as int64 arrays (copies)"""
    return [np.ctypeslib.as_array(t.t[i].count, shape=(int(t.t[i].n_bins),)).astype(np.int64) for i in range(12 if t.have_gc else 4)]


class Device(Batches):
    """bsx_device_* : one HIP device with the index resident in HBM.  Raises if there is no GPU."""

    def __init__(self, ordinal=0):
        L = B.lib()
        self.h = C.c_void_p()
        B.check(L.bsx_device_open(ordinal, C.byref(self.h)), "bsx_device_open")
        names = {"set_opt": "bsx_device_set_opt", "set_reads": "bsx_device_set_reads", "seed_batch": "bsx_seed_batch",
                 "sa_batch": "bsx_sa_batch", "extend_batch": "bsx_extend_batch", "sw_batch": "bsx_sw_batch",
                 "global_batch": "bsx_global_batch"}
        fns = {k: getattr(L, v) for k, v in names.items() if hasattr(L, v)}
        Batches.__init__(self, fns, self.h)
        self.name = L.bsx_device_name(self.h).decode()
        L.bsx_device_n_cu.argtypes = [C.c_void_p]
        self.n_cu = int(L.bsx_device_n_cu(self.h))      # the grids of the persistent kernels are multiples of it

    def upload_index(self, index):
        B.check(B.lib().bsx_device_upload_index(self.h, index.h), "bsx_device_upload_index")

    def build_index(self, index, fill_host=False):
        """both FM indices built on the device from index's pac and left resident (csrc/hip/k_index.hip)"""
        B.check(B.lib().bsx_device_build_index(self.h, index.h, int(fill_host)), "bsx_device_build_index")

    def regions(self, opt, tasks):
        """bsx_regions_batch + bsx_regions_finish: seeding through regions on the device -> (regions, offsets, counts per strand search;
        a negative count = declined)"""
        tasks = np.ascontiguousarray(tasks, dtype=SEED_DT)
        n = len(tasks)
        L = B.lib()
        out, cap, di, dc = C.c_void_p(), C.c_int64(0), C.c_void_p(), C.c_int64(0)
        off = np.zeros(n + 1, dtype=np.int64)
        cnt = np.zeros(n + 1, dtype=np.int32)
        doff = np.zeros(n + 1, dtype=np.int64)
        L.bsx_regions_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_void_p]
        L.bsx_regions_finish.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
        B.check(L.bsx_regions_batch(self.h, C.byref(opt), n, _p(tasks), C.byref(out), C.byref(cap), _p(off), _p(cnt), C.byref(di), C.byref(dc), _p(doff)), "bsx_regions_batch")
        B.check(L.bsx_regions_finish(self.h, C.byref(out), C.byref(cap), _p(off), _p(cnt)), "bsx_regions_finish")
        dt = np.dtype(B.Region)
        tot = int(max([off[i] + cnt[i] for i in range(n) if cnt[i] > 0] + [0]))
        regs = np.frombuffer(C.string_at(out.value, tot * dt.itemsize), dtype=dt).copy() if tot else np.zeros(0, dtype=dt)
        for ptr in (out, di):
            if ptr.value:
                _libc_free(ptr)
        return regs, off[:n], cnt[:n]

    def put_regions(self, regs, off, cnt):
        """bsx_hook_regions_put (tests): regions, offsets and counts of strand searches put where a regions batch leaves its own"""
        regs = np.ascontiguousarray(regs, dtype=np.dtype(B.Region))
        off = np.ascontiguousarray(off, dtype=np.int64)
        cnt = np.ascontiguousarray(cnt, dtype=np.int32)
        assert len(off) == len(cnt)
        f = B.lib().bsx_hook_regions_put
        f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        B.check(f(self.h, len(cnt), _p(regs), len(regs), _p(off), _p(cnt)), "bsx_hook_regions_put")

    def dedup(self, opt, n_reads, per_read):
        """bsx_regions_dedup -> (out_n[n_reads], out_idx[n_reads, bsx_regions_dedup_cap()])"""
        L = B.lib()
        cap = L.bsx_regions_dedup_cap()
        out_n = np.zeros(max(1, n_reads), dtype=np.int32)
        out_idx = np.zeros((max(1, n_reads), cap), dtype=np.uint8)
        L.bsx_regions_dedup.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
        B.check(L.bsx_regions_dedup(self.h, C.byref(opt), n_reads, per_read, _p(out_n), _p(out_idx)), "bsx_regions_dedup")
        return out_n[:n_reads], out_idx[:n_reads]

    def dedup2(self, opt, n_reads, per_read):
        """bsx_regions_dedup2 -> (out_n, out_idx, long_off[n_reads], pool of 16-bit indices the offsets point into)"""
        L = B.lib()
        cap = L.bsx_regions_dedup_cap()
        out_n = np.zeros(max(1, n_reads), dtype=np.int32)
        out_idx = np.zeros((max(1, n_reads), cap), dtype=np.uint8)
        long_off = np.zeros(max(1, n_reads), dtype=np.int64)
        pool, pool_cap = C.c_void_p(), C.c_int64(0)
        L.bsx_regions_dedup2.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        B.check(L.bsx_regions_dedup2(self.h, C.byref(opt), n_reads, per_read, _p(out_n), _p(out_idx), _p(long_off), C.byref(pool), C.byref(pool_cap)), "bsx_regions_dedup2")
        arr = np.frombuffer(C.string_at(pool.value, pool_cap.value * 2), dtype=np.uint16).copy() if pool.value and pool_cap.value else np.zeros(0, dtype=np.uint16)
        if pool.value:
            _libc_free(pool)
        return out_n[:n_reads], out_idx[:n_reads], long_off[:n_reads], arr

    def global_tags(self, jobs, pool_len):
        """bsx_global_batch_tags: K6 plus NM / MD / ZC / ZR of every job with a CIGAR -> (res, pool, tags, [md bytes or None])"""
        jobs = np.ascontiguousarray(jobs, dtype=GLB_DT)
        n = len(jobs)
        res = np.zeros(n, dtype=GLBRES_DT)
        pool = np.zeros(max(1, pool_len), dtype=np.uint32)
        tags = np.zeros(n, dtype=np.dtype(B.GlbTag))
        md = C.c_void_p()
        cap = C.c_int64(0)
        f = B.lib().bsx_global_batch_tags
        f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        B.check(f(self.h, n, _p(jobs), _p(res), _p(pool), pool.size, _p(tags), C.byref(md), C.byref(cap)), "bsx_global_batch_tags")
        out = []
        for k in range(n):
            if tags[k]["l_md"] < 0:
                out.append(None)
            else:
                out.append(C.string_at(md.value + int(tags[k]["md_off"]), int(tags[k]["l_md"]) + 1))
        if md.value:
            _libc_free(md)
        return res, pool, tags, out

    def global_tags_ctx(self, jobs, pool_len):
        """bsx_global_batch_tags_ctx: the above plus, per job, the retention / conversion counts by cytosine context of both bisulfite-strand
        hypotheses -> (res, pool, tags, [md], ctx[n, 2, 5, 2] uint16: [strand][A, C, G, T, N context][retained, converted])"""
        jobs = np.ascontiguousarray(jobs, dtype=GLB_DT)
        n = len(jobs)
        res = np.zeros(n, dtype=GLBRES_DT)
        pool = np.zeros(max(1, pool_len), dtype=np.uint32)
        tags = np.zeros(n, dtype=np.dtype(B.GlbTag))
        ctx = np.zeros((n, 2, 5, 2), dtype=np.uint16)
        md = C.c_void_p()
        cap = C.c_int64(0)
        f = B.lib().bsx_global_batch_tags_ctx
        f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_void_p]
        B.check(f(self.h, n, _p(jobs), _p(res), _p(pool), pool.size, _p(tags), C.byref(md), C.byref(cap), _p(ctx)), "bsx_global_batch_tags_ctx")
        out = [None if tags[k]["l_md"] < 0 else C.string_at(md.value + int(tags[k]["md_off"]), int(tags[k]["l_md"]) + 1) for k in range(n)]
        if md.value:
            _libc_free(md)
        return res, pool, tags, out, ctx

    def qc_batch(self, jobs, pool):
        """bsx_qc_batch: the BISCUITqc column counts of the jobs (array of _lib.QcJob's layout; pool: their CIGAR words) added to the device's table"""
        jobs = np.ascontiguousarray(jobs, dtype=np.dtype(B.QcJob))
        pool = np.ascontiguousarray(pool, dtype=np.uint32)
        f = B.lib().bsx_qc_batch
        f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t]
        B.check(f(self.h, len(jobs), _p(jobs), _p(pool), pool.size), "bsx_qc_batch")

    def qc_read(self, reset=False):
        """bsx_qc_read -> (readpos[2, 2, 301, 2], conv[8], confusion[16]) as int64 arrays"""
        c = B.QcCounts()
        f = B.lib().bsx_qc_read
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        B.check(f(self.h, C.byref(c), int(reset)), "bsx_qc_read")
        return (np.array(c.readpos, dtype=np.int64).reshape(2, 2, 301, 2), np.array(c.conv, dtype=np.int64), np.array(c.confusion, dtype=np.int64))

    def cov_batch(self, jobs, pool):
        """bsx_cov_batch: the M runs of the jobs with QC_COV (array of _lib.QcJob's layout; pool: their CIGAR words) added to the device's depth state"""
        jobs = np.ascontiguousarray(jobs, dtype=np.dtype(B.QcJob))
        pool = np.ascontiguousarray(pool, dtype=np.uint32)
        f = B.lib().bsx_cov_batch
        f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t]
        B.check(f(self.h, len(jobs), _p(jobs), _p(pool), pool.size), "bsx_cov_batch")

    def cov_set_mask(self, which, intervals):
        """bsx_cov_set_mask: mask `which` (_lib.COV_MASK_TOPGC / _BOTGC) = the union of the half-open intervals [(beg, end)] of forward coordinates"""
        iv = np.ascontiguousarray(intervals, dtype=np.int64).reshape(-1, 2)
        f = B.lib().bsx_cov_set_mask
        f.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
        B.check(f(self.h, int(which), len(iv), _p(iv) if len(iv) else None), "bsx_cov_set_mask")

    def cov_tables(self):
        """bsx_cov_tables -> twelve int64 arrays count[depth] (four without the masks), in the order of _lib.CovTables"""
        t = B.CovTables()
        L = B.lib()
        L.bsx_cov_tables.argtypes = [C.c_void_p, C.c_void_p]
        L.bsx_cov_tables_free.argtypes = [C.c_void_p]
        L.bsx_cov_tables_free.restype = None
        B.check(L.bsx_cov_tables(self.h, C.byref(t)), "bsx_cov_tables")
        try:
            return cov_tables_arrays(t)
        finally:
            L.bsx_cov_tables_free(C.byref(t))

    def cov_reset(self):
        """bsx_cov_reset: the depth state and both masks freed"""
        f = B.lib().bsx_cov_reset
        f.argtypes = [C.c_void_p]
        B.check(f(self.h), "bsx_cov_reset")

    def meth_batch(self, jobs, pool):
        """bsx_meth_batch: the columns of the jobs (array of _lib.MethJob's layout; pool: their CIGAR words and quality masks) added to the device's
        four counters per position; the reads are those of set_reads"""
        jobs = np.ascontiguousarray(jobs, dtype=np.dtype(B.MethJob))
        pool = np.ascontiguousarray(pool, dtype=np.uint32)
        f = B.lib().bsx_meth_batch
        f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t]
        B.check(f(self.h, len(jobs), _p(jobs), _p(pool), pool.size), "bsx_meth_batch")

    def meth_read(self, fpos, n):
        """bsx_meth_read -> int64[n, 4]: ret, conv, opp_ref, opp_alt of the positions [fpos, fpos + n)"""
        out = np.zeros((int(n), 4), np.uint32)
        f = B.lib().bsx_meth_read
        f.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        B.check(f(self.h, int(fpos), int(n), _p(out)), "bsx_meth_read")
        return out.astype(np.int64)

    def meth_tables(self):
        """bsx_meth_tables -> (K[5], S[5]) as int64 arrays: reported sites and the sum of their betas in thousandths for CA, CC, CG, CT, CN"""
        t = B.MethTables()
        f = B.lib().bsx_meth_tables
        f.argtypes = [C.c_void_p, C.c_void_p]
        B.check(f(self.h, C.byref(t)), "bsx_meth_tables")
        return np.array(t.k, dtype=np.int64), np.array(t.s, dtype=np.int64)

    def meth_reset(self):
        """bsx_meth_reset: the counters freed"""
        f = B.lib().bsx_meth_reset
        f.argtypes = [C.c_void_p]
        B.check(f(self.h), "bsx_meth_reset")

    def meth_sites_window(self, f_lo, f_hi, typ="cg", min_cov=1, merge=False, cap=1 << 20):
        """bsx_meth_sites, one call -> (records, f_next): the records (numpy structured array of _lib.MethSite's layout) of as many whole tiles
        of [f_lo, f_hi) from f_lo on as fit cap records, and where the next call goes on (f_hi: nothing is left)"""
        opt = B.MethSiteOpt(B.METH_TYPES[typ], int(bool(merge)), int(min_cov), 0)
        out = np.zeros(max(int(cap), 0), dtype=np.dtype(B.MethSite))
        n, f_next = C.c_int64(-1), C.c_int64(-1)
        f = B.lib().bsx_meth_sites
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        B.check(f(self.h, C.byref(opt), int(f_lo), int(f_hi), _p(out), int(cap), C.byref(n), C.byref(f_next)), "bsx_meth_sites")
        return out[:n.value].copy(), f_next.value

    def meth_sites(self, f_lo, f_hi, typ="cg", min_cov=1, merge=False, cap=1 << 20):
        """the methylation sites of the device's counters that belong to [f_lo, f_hi) (k_msite.hip) -> numpy structured array of _lib.MethSite's
        layout in ascending position: what `biscuit pileup` -> `biscuit vcf2bed -t typ -k min_cov` lists, with merge what `biscuit mergecg`
        makes of it (typ cg only); window by window through a buffer of cap records (at least _lib.COV_TILE)"""
        parts = []
        while True:
            recs, f_next = self.meth_sites_window(f_lo, f_hi, typ, min_cov, merge, cap)
            parts.append(recs)
            if f_next >= f_hi:
                return np.concatenate(parts)
            assert f_next > f_lo
            f_lo = f_next

    def markdup_batch(self, keys, first_ordinal):
        """bsx_markdup_batch: keys = uint64[n, 2] (_lib.MarkdupKey's layout; both words all ones: skipped), the template with ordinal
        first_ordinal + i at keys[i] -> uint8[n], 1 where an equal key with a lower ordinal is in the device's table or earlier in the batch"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, 2)
        out = np.zeros(len(keys), np.uint8)
        f = B.lib().bsx_markdup_batch
        f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p]
        B.check(f(self.h, len(keys), _p(keys), int(first_ordinal), _p(out)), "bsx_markdup_batch")
        return out

    def markdup_reset(self):
        """bsx_markdup_reset: the device's table of template keys emptied"""
        f = B.lib().bsx_markdup_reset
        f.argtypes = [C.c_void_p]
        B.check(f(self.h), "bsx_markdup_reset")

    def markdup_table(self):
        """bsx_markdup_table_info (tests, diagnostics) -> (slots, slots taken)"""
        n, u = C.c_uint64(), C.c_uint64()
        f = B.lib().bsx_markdup_table_info
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        B.check(f(self.h, C.byref(n), C.byref(u)), "bsx_markdup_table_info")
        return n.value, u.value

    def sort_run(self, keys):
        """bsx_sort_run: keys = uint64[n] (_lib.sort_key) -> uint32[n], perm[i] = index of the i-th key in stable order; the sorted keys stay on the
        device as the next run"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
        perm = np.zeros(len(keys), np.uint32)
        f = B.lib().bsx_sort_run
        f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        B.check(f(self.h, len(keys), _p(keys) if len(keys) else None, _p(perm) if len(keys) else None), "bsx_sort_run")
        return perm

    def sort_schedule(self):
        """bsx_sort_schedule -> uint32[total], the run every position of the stable sort of all retained keys (runs concatenated in run order) comes from"""
        n, out = C.c_int64(0), C.c_void_p()
        f = B.lib().bsx_sort_schedule
        f.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_void_p)]
        B.check(f(self.h, C.byref(n), C.byref(out)), "bsx_sort_schedule")
        if not out.value:
            return np.zeros(0, np.uint32)
        try:
            return np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint32)), shape=(n.value,)).copy()
        finally:
            _libc_free(out)

    def bam_encode(self, header, text):
        """bsx_bam_encode on the device (k_bam.hip): SAM text (bytes, whole lines) under the @SQ lines of `header` (bytes) -> (the BAM records,
        the 0-based index of the first refused line or -1, its _lib.BAM_E_* or 0); the records before a refused line are returned"""
        return bam_encode(self.h, header, text)

    def bgzf_deflate(self, payload):
        """bsx_bgzf_deflate on the device (k_bgzf.hip): bytes -> the BGZF members of its 0xff00-byte blocks, behind each other (no EOF block)"""
        return bgzf_deflate(self.h, payload)

    def sort_info(self):
        """bsx_sort_info -> (runs, keys) retained on the device"""
        r, k = C.c_uint64(), C.c_uint64()
        f = B.lib().bsx_sort_info
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        B.check(f(self.h, C.byref(r), C.byref(k)), "bsx_sort_info")
        return r.value, k.value

    def sort_reset(self):
        """bsx_sort_reset: every retained run freed"""
        f = B.lib().bsx_sort_reset
        f.argtypes = [C.c_void_p]
        B.check(f(self.h), "bsx_sort_reset")

    def counters(self, reset=False):
        c = (C.c_uint64 * 4)()
        B.check(B.lib().bsx_device_counters(self.h, c, int(reset)), "bsx_device_counters")
        return list(c)

    def seed_passes(self, reset=False):
        """([FM blocks, table entries] of the first seeding pass, [FM blocks, table entries, launches, strand searches] of the second pass
        inside the chunk's sequence, [ms first pass, ms second pass]) since the last reset; read before counters()/seed_table() with reset"""
        w = (C.c_uint64 * 6)()
        ms = (C.c_double * 2)()
        B.check(B.lib().bsx_device_seed_passes(self.h, w, ms, int(reset)), "bsx_device_seed_passes")
        return list(w[:2]), list(w[2:]), list(ms)

    def region_work(self, reset=False):
        """[strand searches, SA intervals, occurrences looked up, regions written, read bases] of the region kernels since the last reset"""
        w = (C.c_uint64 * 5)()
        B.check(B.lib().bsx_device_region_work(self.h, w, int(reset)), "bsx_device_region_work")
        return list(w)

    def seed_table(self, reset=False):
        """(table entries read by the seeding kernel since the last reset, depth K of the resident table of k-mer intervals; 0 = none)"""
        n, k = C.c_uint64(), C.c_int()
        B.check(B.lib().bsx_device_seed_table(self.h, C.byref(n), C.byref(k), int(reset)), "bsx_device_seed_table")
        return int(n.value), int(k.value)

    def kernel_time(self, k, reset=False):
        ms = C.c_double()
        n = C.c_int64()
        B.check(B.lib().bsx_device_kernel_time(self.h, k, C.byref(ms), C.byref(n), int(reset)), "bsx_device_kernel_time")
        return ms.value, n.value

    def close(self):
        if self.h:
            B.lib().bsx_device_close(self.h)
            self.h = None
