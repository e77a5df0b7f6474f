"""Writes tests/golden/ext_stop.npz: the designed jobs of tests/ext_stop_cases.py and the six outputs of the reference's own ksw_extend2
(oracle/_ref, built by `make ref`) for each of them.  Run from the repository root: python tests/golden/make_vectors_ext_stop.py"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ext_pk_cases as P      # noqa: E402
import ext_stop_cases as X    # noqa: E402
import oracle_lib             # noqa: E402


def main():
    R = oracle_lib.ref_lib()
    if R is None:
        sys.exit("oracle/_ref has not been built (make ref)")
    cases = X.build()
    answers = []
    for si, fam, parent, w, eb, h0, q, t in cases:
        a, b, gp, zd = X.scorings()[si]
        o = P.opt_of(a, b, gp, zd)
        out = (C.c_int * 6)()
        R.ref_ksw_extend2(C.c_int(len(q)), X._p(q), C.c_int(len(t)), X._p(t), o.ctmat if parent else o.gamat, C.c_int(gp[0]), C.c_int(gp[1]),
                          C.c_int(gp[2]), C.c_int(gp[3]), C.c_int(w), C.c_int(eb), C.c_int(zd), C.c_int(h0), out)
        answers.append(list(out))
    X.save(X.GOLDEN, cases, answers)
    by = {}
    for c in cases:
        by[(c[0], c[1])] = by.get((c[0], c[1]), 0) + 1
    print(len(cases), "jobs;", {f: sum(v for (s, ff), v in by.items() if ff == f) for f in X.FAMILIES})


if __name__ == "__main__":
    main()
