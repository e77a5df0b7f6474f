/* bam_rec.h -- one SAM line -> one BAM record (tests/bam_model.py): the one statement of the record rule, compiled
 * for the host by bam.c and for the device by k_bam.hip (BAM_FN = __device__ there).  Plain C, no library call, no table in memory but
 * the caller's reference names: bam_rec_encode(out = NULL) is the size pass, the same call with a buffer is the emit pass, so the two
 * cannot disagree.  Bytes are stored one at a time: on the device every store is a vector store of a byte. */
#ifndef BSX_BAM_REC_H
#define BSX_BAM_REC_H
#include <stdint.h>

#ifndef BAM_FN
#define BAM_FN static inline
#endif

/* the reference names of the header, sorted bytewise (a prefix before the longer name): name k is names[off[k] .. off[k + 1]), id[k] the
 * index of the first @SQ line that has it */
typedef struct bam_reftab { const char *names; const uint32_t *off; const int32_t *id; int32_t n; } bam_reftab_t;

BAM_FN int32_t bam_ref_find(const bam_reftab_t *T, const char *s, uint32_t len)   /* -2: no such name */
{
	int32_t lo = 0, hi = T->n - 1, found = -2;
	while (lo <= hi && found == -2) {
		const int32_t mid = lo + ((hi - lo) >> 1);
		const char *m = T->names + T->off[mid];
		const uint32_t ml = T->off[mid + 1] - T->off[mid], k = ml < len ? ml : len;
		uint32_t i = 0;
		int c;
		while (i < k && m[i] == s[i]) ++i;
		c = i < k ? ((unsigned char)m[i] < (unsigned char)s[i] ? -1 : 1) : ml < len ? -1 : ml > len ? 1 : 0;
		if (c == 0) found = T->id[mid];
		else if (c < 0) lo = mid + 1; else hi = mid - 1;
	}
	return found;
}

/* [-+]digits (sign: only when `sign`), at most 18 digits; 0: not a number.  (No early exit, here or below: on the device every exit taken by
 * some lanes of a wave costs a mask, and a parse with dozens of them runs out of scalar registers.) */
BAM_FN int bam_parse_int(const char *s, uint32_t len, int sign, int64_t *v)
{
	uint32_t i = 0;
	int neg = 0, ok;
	uint64_t x = 0;
	if (sign && len && (s[0] == '-' || s[0] == '+')) { neg = s[0] == '-'; i = 1; }
	ok = i < len && len - i <= 18;
	if (ok) for (; i < len; ++i) {
		const uint32_t d = (uint32_t)(unsigned char)s[i] - (uint32_t)'0';
		ok &= d <= 9;
		x = x * 10 + d;
	}
	*v = neg ? -(int64_t)x : (int64_t)x;
	return ok;
}

BAM_FN int bam_reg2bin(int64_t beg, int64_t end)   /* the specification's, on arithmetic shifts */
{
	--end;
	if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
	if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
	if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
	if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
	if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
	return 0;
}

BAM_FN int bam_cigar_op(char c)
{
	switch (c) {
	case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
	case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8;
	}
	return -1;
}

BAM_FN int bam_seq_code(char c)
{
	switch (c) {
	case '=': return 0; case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5;
	case 'S': return 6; case 'V': return 7; case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11;
	case 'K': return 12; case 'D': return 13; case 'B': return 14;
	}
	return 15;
}

/* the record of line[0 .. len) (no newline), block_size included: its length, written to out when out != NULL; 0 and *err = BSX_BAM_E_*
 * when the line is refused.  A refusal is noted (the first one counts) and the walk goes on to the end of the line -- reads stay inside the
 * line, and a caller passes a buffer only for a line the size pass has taken.  size_out != NULL: the length is also stored there when the line
 * is taken (the device's caller reads both results from memory). */
BAM_FN uint32_t bam_rec_encode(const char *line, uint32_t len, const bam_reftab_t *T, uint8_t *out, int *err, uint32_t *size_out)
{
#define BAM_PUT(b) do { if (out) out[n] = (uint8_t)(b); ++n; } while (0)
#define BAM_PUT32(v) do { const uint32_t v_ = (uint32_t)(v); BAM_PUT(v_); BAM_PUT(v_ >> 8); BAM_PUT(v_ >> 16); BAM_PUT(v_ >> 24); } while (0)
#define BAM_PUT16(v) do { const uint32_t w_ = (uint32_t)(v); BAM_PUT(w_); BAM_PUT(w_ >> 8); } while (0)
#define BAM_BAD(e) do { if (!bad) bad = (e); } while (0)
	uint32_t fb[12], i, n = 0, n_cig = 0, l_seq, at;   /* fb[j]: where column j begins; fb[11]: one past the 11th column's tab (or len + 1) */
	int64_t flag, pos, mapq, pnext, tlen, reflen = 0, L;
	int32_t rid, nid;
	int bad = 0, few = 0, qstar;
	/* (fb is only ever indexed by constants, so that it lives in registers on the device) */
#define BAM_NEXT(j) do { uint32_t p_ = fb[(j) - 1]; while (p_ < len && line[p_] != '\t') ++p_; \
		if (p_ < len) fb[j] = p_ + 1; else { fb[j] = len + 1; if ((j) < 11) few = 1; } } while (0)
#define BAM_EMPTY(j) (fb[(j) + 1] - fb[j] < 2)
	fb[0] = 0;
	BAM_NEXT(1); BAM_NEXT(2); BAM_NEXT(3); BAM_NEXT(4); BAM_NEXT(5); BAM_NEXT(6); BAM_NEXT(7); BAM_NEXT(8); BAM_NEXT(9); BAM_NEXT(10); BAM_NEXT(11);
	if (few || BAM_EMPTY(0) || BAM_EMPTY(1) || BAM_EMPTY(2) || BAM_EMPTY(3) || BAM_EMPTY(4) || BAM_EMPTY(5) || BAM_EMPTY(6) || BAM_EMPTY(7) || BAM_EMPTY(8) ||
	    BAM_EMPTY(9) || BAM_EMPTY(10)) { *err = 1; if (size_out) *size_out = 0; return 0; }   /* fewer than 11 columns, or an empty one: the one early exit */
#undef BAM_NEXT
#undef BAM_EMPTY
#define COL(j) (line + fb[j])
#define CLEN(j) (fb[(j) + 1] - fb[j] - 1)
	if (!(bam_parse_int(COL(1), CLEN(1), 0, &flag) & bam_parse_int(COL(3), CLEN(3), 1, &pos) & bam_parse_int(COL(4), CLEN(4), 0, &mapq) &
	      bam_parse_int(COL(7), CLEN(7), 1, &pnext) & bam_parse_int(COL(8), CLEN(8), 1, &tlen))) BAM_BAD(1);
	if (flag > 65535 || mapq > 255 || pos <= -((int64_t)1 << 31) || pos > ((int64_t)1 << 31) || pnext <= -((int64_t)1 << 31) || pnext > ((int64_t)1 << 31) ||
	    tlen < -((int64_t)1 << 31) || tlen >= ((int64_t)1 << 31)) BAM_BAD(1);
	if (CLEN(0) > 254) BAM_BAD(4);
	if (!(CLEN(5) == 1 && COL(5)[0] == '*')) {
		const char *c = COL(5);
		uint32_t v = 0;
		int have = 0;
		for (i = 0; i < CLEN(5); ++i) {
			if (c[i] >= '0' && c[i] <= '9') { v = v * 10 + (uint32_t)(c[i] - '0'); have = 1; if (v >= 1u << 28) { BAM_BAD(1); v = 0; } }
			else {
				const int op = bam_cigar_op(c[i]);
				if (op < 0 || !have) BAM_BAD(1);
				if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) reflen += v;
				++n_cig; v = 0; have = 0;
			}
		}
		if (have) BAM_BAD(1);
		if (n_cig > 65535) BAM_BAD(5);
	}
	rid = CLEN(2) == 1 && COL(2)[0] == '*' ? -1 : bam_ref_find(T, COL(2), CLEN(2));
	if (rid == -2) BAM_BAD(6);
	nid = CLEN(6) == 1 && COL(6)[0] == '=' ? rid : CLEN(6) == 1 && COL(6)[0] == '*' ? -1 : bam_ref_find(T, COL(6), CLEN(6));
	if (nid == -2) BAM_BAD(6);
	l_seq = CLEN(9) == 1 && COL(9)[0] == '*' ? 0 : CLEN(9);
	qstar = CLEN(10) == 1 && COL(10)[0] == '*';
	if (!qstar && CLEN(10) != l_seq) BAM_BAD(7);
	L = ((flag & 4) || n_cig == 0 || reflen == 0) ? 1 : reflen;
	BAM_PUT32(0);   /* block_size: filled in last */
	BAM_PUT32(rid); BAM_PUT32(pos - 1);
	BAM_PUT(CLEN(0) + 1); BAM_PUT(mapq); BAM_PUT16(bam_reg2bin(pos - 1, pos - 1 + L));
	BAM_PUT16(n_cig); BAM_PUT16(flag); BAM_PUT32(l_seq); BAM_PUT32(nid); BAM_PUT32(pnext - 1); BAM_PUT32(tlen);
	for (i = 0; i < CLEN(0); ++i) BAM_PUT(COL(0)[i]);
	BAM_PUT(0);
	if (n_cig) {
		const char *c = COL(5);
		uint32_t v = 0;
		for (i = 0; i < CLEN(5); ++i) {
			if (c[i] >= '0' && c[i] <= '9') v = v * 10 + (uint32_t)(c[i] - '0');
			else { BAM_PUT32(v << 4 | (uint32_t)bam_cigar_op(c[i])); v = 0; }
		}
	}
	for (i = 0; i + 1 < l_seq; i += 2) BAM_PUT(bam_seq_code(COL(9)[i]) << 4 | bam_seq_code(COL(9)[i + 1]));
	if (i < l_seq) BAM_PUT(bam_seq_code(COL(9)[i]) << 4);
	if (qstar) for (i = 0; i < l_seq; ++i) BAM_PUT(0xff);
	else for (i = 0; i < CLEN(10); ++i) BAM_PUT(COL(10)[i] - 33);
	for (at = fb[11]; at <= len; ) { /* the optional fields */
		const char *f = line + at, *v;
		uint32_t fl = 0, vl;
		while (at + fl < len && f[fl] != '\t') ++fl;
		at += fl + 1;
		if (fl < 5) { BAM_BAD(2); continue; }
		if (f[2] != ':' || f[4] != ':') BAM_BAD(2);
		v = f + 5; vl = fl - 5;
		if (f[3] == 'A') {
			if (vl != 1) BAM_BAD(2);
			else { BAM_PUT(f[0]); BAM_PUT(f[1]); BAM_PUT('A'); BAM_PUT(v[0]); }
		} else if (f[3] == 'Z') {
			BAM_PUT(f[0]); BAM_PUT(f[1]); BAM_PUT('Z');
			for (i = 0; i < vl; ++i) BAM_PUT(v[i]);
			BAM_PUT(0);
		} else if (f[3] == 'i') {
			const uint32_t s = vl && (v[0] == '-' || v[0] == '+') ? 1 : 0;
			int64_t x = 0;
			int digits = s < vl;
			for (i = s; i < vl; ++i) digits &= v[i] >= '0' && v[i] <= '9';
			if (!digits) BAM_BAD(2);
			else if (!bam_parse_int(v, vl, 1, &x) || x < -((int64_t)1 << 31) || x > ((int64_t)1 << 32) - 1) BAM_BAD(3);
			BAM_PUT(f[0]); BAM_PUT(f[1]);
			if (x < 0) {
				if (x >= -128) { BAM_PUT('c'); BAM_PUT(x); }
				else if (x >= -32768) { BAM_PUT('s'); BAM_PUT16(x); }
				else { BAM_PUT('i'); BAM_PUT32(x); }
			} else {
				if (x <= 255) { BAM_PUT('C'); BAM_PUT(x); }
				else if (x <= 65535) { BAM_PUT('S'); BAM_PUT16(x); }
				else { BAM_PUT('I'); BAM_PUT32(x); }
			}
		} else if (f[3] == 'f') { /* [-]digits[.digits]: the integer of all digits over 10^(digits behind the point), both exact in double */
			const uint32_t s = vl && v[0] == '-' ? 1 : 0;
			uint32_t nfrac = 0, nint = 0;
			int dot = 0;
			uint64_t m = 0;
			double x, p10 = 1.0;
			union { float f; uint32_t u; } cv;
			for (i = s; i < vl; ++i) {
				if (v[i] == '.' && !dot) dot = 1;
				else if (v[i] < '0' || v[i] > '9' || m >= 100000000000000ull) BAM_BAD(2);   /* no digit, or it would make 10^15 or more */
				else { m = m * 10 + (uint64_t)(v[i] - '0'); if (dot) ++nfrac; else ++nint; }
			}
			if (!nint || (dot && !nfrac) || nfrac > 22) { BAM_BAD(2); nfrac = 0; }
			for (i = 0; i < nfrac; ++i) p10 *= 10.0;   /* exact up to 10^22 */
			x = (double)m / p10;
			cv.f = (float)(s ? -x : x);
			BAM_PUT(f[0]); BAM_PUT(f[1]); BAM_PUT('f'); BAM_PUT32(cv.u);
		} else BAM_BAD(2);
	}
	*err = bad;
	if (bad) n = 0;
	if (size_out) *size_out = n;
	if (out && !bad) { const uint32_t bs = n - 4; out[0] = (uint8_t)bs; out[1] = (uint8_t)(bs >> 8); out[2] = (uint8_t)(bs >> 16); out[3] = (uint8_t)(bs >> 24); }
	return n;
#undef COL
#undef CLEN
#undef BAM_PUT
#undef BAM_PUT32
#undef BAM_PUT16
#undef BAM_BAD
}

#endif
