"""A plain Smith-Waterman score in int64 numpy: the reference of the seed filter's alignment (ksw_align2 in 16-bit mode, score only).
Rows are target bases, columns are query bases; mat is indexed [target * 5 + query].

    Ht[j] = max(0, H[j-1] + mat[t*5 + q[j]], E[j])
    F[j]  = max over k < j of Ht[k] - o_ins - (j - k) * e_ins
    H'[j] = max(Ht[j], F[j])
    E'[j] = max(E[j] - e_del, H'[j] - o_del - e_del)

The score is the largest H'.  No striping, no 16-bit arithmetic, no bias: nothing of the kernels' layout."""
import numpy as np

NEG = -(1 << 40)


def sw_score(q, t, mat, o_del, e_del, o_ins, e_ins, insertions=True, deletions=True):
    """insertions / deletions = False forbids that kind of gap (what a vector's path needs is shown by the score dropping)"""
    q = np.asarray(q, np.int64)
    t = np.asarray(t, np.int64)
    m = np.asarray(mat, np.int64).reshape(5, 5)
    n = len(q)
    if n == 0 or len(t) == 0:
        return 0
    jj = np.arange(n, dtype=np.int64)
    H = np.zeros(n, np.int64)
    E = np.full(n, NEG, np.int64)
    best = 0
    for tb in t:
        diag = np.concatenate(([0], H[:-1]))
        Ht = np.maximum(0, np.maximum(diag + m[tb, q], E))
        F = np.full(n, NEG, np.int64)
        if insertions and n > 1:
            F[1:] = np.maximum.accumulate(Ht + jj * e_ins)[:-1] - o_ins - jj[1:] * e_ins
        H = np.maximum(Ht, F)
        E = np.maximum(E - e_del, H - o_del - e_del) if deletions else E
        best = max(best, int(H.max()))
    return best
