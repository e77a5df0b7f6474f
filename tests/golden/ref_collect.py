"""mem_collect_intv (memchain.c:50-106) for the generators of the recorded vectors (make_vectors.py, make_vectors_seed.py).  The function is
static in a file that does not build here, so its 20-line driver is restated below over the REAL bwt_smem1a / bwt_seed_strategy1 (all FM
work is the reference's, through oracle/_ref/libbiscuit_ref.so); the result is what the seeding kernel must return for the read, interval
for interval."""
import ctypes as C
import numpy as np

u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)


def P(a, t):
    return a.ctypes.data_as(t)


def collect_intv(R, H, par, conv, min_seed_len=19, split_factor=1.5, split_width=10, max_mem_intv=20, start_width=1, cap=1024, stats=None):
    """R: the reference library; H: {parent: its bwt handle}; conv: the converted read.  cap: entries of the buffer bwt_smem1a's list is
    copied to (asserted not to be exceeded).  stats: a dict that receives what the reference saw -- the SMEMs pass 1 kept, the indices of
    those pass 2 re-seeded, the seeds of pass 3, the largest x2.  -> (n, 4) uint64 ordered by info"""
    L_ = len(conv)
    split_len = int(min_seed_len * split_factor + .499)
    mem = []
    o1 = np.zeros(4 * cap, np.uint64); r1 = C.c_int()

    def smem1(x, mi):
        n1 = R.ref_bwt_smem1a(H[par], H[1 - par], L_, P(conv, u8p), x, mi, C.c_uint64(0), P(o1, u64p), cap, C.byref(r1))
        assert n1 <= cap
        return [tuple(int(v) for v in o1[4 * i:4 * i + 4]) for i in range(n1)], r1.value
    x = 0
    while x < L_:                                    # pass 1 (memchain.c:65-73)
        if conv[x] < 4:
            got, x = smem1(x, start_width)
            mem += [m for m in got if (m[3] & 0xffffffff) - (m[3] >> 32) >= min_seed_len]
        else:
            x += 1
    n_pass1, reseeded = len(mem), []
    for k in range(len(mem)):                        # pass 2 (memchain.c:76-85)
        st, en = mem[k][3] >> 32, mem[k][3] & 0xffffffff
        if en - st < split_len or mem[k][2] > split_width:
            continue
        reseeded.append(k)
        got, _ = smem1((st + en) >> 1, mem[k][2] + 1)
        mem += [m for m in got if (m[3] & 0xffffffff) - (m[3] >> 32) >= min_seed_len]
    n_pass2 = len(mem)
    x = 0
    a1 = np.zeros(4, np.uint64)
    while max_mem_intv > 0 and x < L_:               # pass 3 (memchain.c:88-103)
        if conv[x] < 4:
            x = R.ref_bwt_seed_strategy1(H[par], H[1 - par], L_, P(conv, u8p), x, min_seed_len, max_mem_intv, P(a1, u64p))
            if int(a1[2]) > 0:
                mem.append(tuple(int(v) for v in a1))
        else:
            x += 1
    if stats is not None:
        stats.update(pass1=n_pass1, reseeded=reseeded, reseeded_len=[(mem[k][3] & 0xffffffff) - (mem[k][3] >> 32) for k in reseeded],
                     reseeded_x2=[mem[k][2] for k in reseeded], pass3=len(mem) - n_pass2, pass3_x2=[m[2] for m in mem[n_pass2:]],
                     max_x2=max([m[2] for m in mem] + [0]))
    mem.sort(key=lambda m: m[3])                     # ks_introsort(mem_intv): records with equal info are identical
    return np.array(mem, np.uint64).reshape(-1, 4)
