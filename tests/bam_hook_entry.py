"""Child process of tests/test_gpu_bam.py: the product's command line (bsx_align_main, the HIP device) under an emit hook.  argv[1]: where the
pieces the hook was handed are written, behind each other; the rest: the command line.  The header's piece must come first, with index -1, the
others must count from 0.  Exit status: the command line's."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from biscuit_amd import _lib
    L = _lib.lib()
    pieces = []
    HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t)

    def emit(ud, idx, text, n):
        pieces.append((idx, C.string_at(text, n) if n else b""))

    hook = HOOK(emit)
    C.c_void_p.in_dll(L, "bsx_emit_hook").value = C.cast(hook, C.c_void_p).value
    args = [b"biscuit_align"] + [a.encode() for a in sys.argv[2:]]
    arr = (C.c_char_p * (len(args) + 1))(*args, None)
    rc = L.bsx_align_main(len(args), arr)
    C.c_void_p.in_dll(L, "bsx_emit_hook").value = None
    if rc == 0 and [i for i, _ in pieces] != [-1] + list(range(len(pieces) - 1)):
        sys.stderr.write("piece indices: %r\n" % ([i for i, _ in pieces][:20],))
        return 3
    with open(sys.argv[1], "wb") as f:
        f.write(b"".join(p for _, p in pieces))
    return rc


if __name__ == "__main__":
    sys.exit(main())
