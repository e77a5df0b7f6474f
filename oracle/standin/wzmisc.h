/* oracle/standin/wzmisc.h -- TEST INFRASTRUCTURE.  The reference's memchain.c includes a header of this name from a library that is not
 * vendored with it and takes one name from it: min, on two ints (memchain.c:779-787, the band of an extension).  This project's own
 * statement of that one name; see oracle/ref_shim.c. */
#ifndef BSX_STANDIN_WZMISC_H
#define BSX_STANDIN_WZMISC_H
#ifndef min
#define min(a, b) ((a) < (b) ? (a) : (b))
#endif
#endif
