/* oracle/standin/encode.h -- TEST INFRASTRUCTURE.  The reference's bntseq.c includes a header of this name from a library that is
 * not vendored with it and uses nothing of it: empty on purpose (see oracle/ref_shim.c). */
