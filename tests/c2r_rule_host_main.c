/* The rules of mem_chain2region (biscuit_amd/csrc/host/c2r_rule.h) on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer
 * (tests/test_c2r_rule_host.py builds and runs this).  Every table row is a designed input with the value worked out by hand from the
 * reference's lines (lib/aln/memchain.c, cited at each table): the edges at which one of the copies of a rule could have drifted.
 * The genome of the window rows: l_pac = 1000, two contigs [0, 400) and [400, 1000); on the reverse strand they lie at [1600, 2000)
 * and [1000, 1600).  Prints "ok". */
#include <stdio.h>
#include <stdint.h>
#include "c2r_rule.h"

#define N(a) ((int)(sizeof(a) / sizeof((a)[0])))
#define FAIL(what, i) do { fprintf(stderr, "%s:%d: %s row %d\n", __FILE__, __LINE__, what, i); return 1; } while (0)
#define LP 1000

int main(void)
{
	int i;
	/* memchain.c:593-594: b = rbeg - (qbeg + gap), e = rbeg + len + ((l_query - qbeg - len) + gap) */
	static const struct { int64_t rbeg; int qbeg, len, lq, gl, gr; int64_t b, e; } span[] = {
		{500, 10, 20, 50, 7, 9, 483, 549},
		{100, 0, 30, 50, 1, 11, 99, 161},     /* starts the read */
		{100, 20, 30, 50, 11, 1, 69, 131},    /* ends it */
		{100, 0, 50, 50, 1, 1, 99, 151},      /* spans it */
	};
	/* memchain.c:599-604, then bns_fetch_seq's clamp to the chain's contig (memchain.c:889) */
	static const struct { int64_t r0, r1, pos, cb, ce, x0, x1; } win[] = {
		{950, 1060, 980, 400, 1000, 950, 1000},      /* straddles l_pac, forward chain: the reverse half goes */
		{950, 1060, 1010, 400, 1000, 1000, 1060},    /* the same window, reverse chain: the forward half goes; contig mirrored to [1000, 1600) */
		{1580, 1700, 1650, 0, 400, 1600, 1700},      /* reverse strand, first contig = [1600, 2000): clamped on the left */
		{1500, 1650, 1550, 400, 1000, 1500, 1600},   /* reverse strand, last contig = [1000, 1600): clamped on the right */
		{-30, 80, 20, 0, 400, 0, 80},                /* rmax0 < 0 */
		{1950, 2040, 1960, 0, 400, 1950, 2000},      /* rmax1 > 2 l_pac */
		{350, 460, 380, 0, 400, 350, 400},           /* forward strand, the contig's end inside the window */
		{380, 460, 420, 400, 1000, 400, 460},        /* and the next contig's start */
		{1000, 1100, 1050, 400, 1000, 1000, 1100},   /* rmax0 == l_pac: not a straddle */
		{900, 1000, 950, 400, 1000, 900, 1000},      /* rmax1 == l_pac: neither */
		{350, 460, 380, 0, 2 * LP, 350, 460},        /* no contig given (the host clamps to it afterwards): forward */
		{1580, 1700, 1650, 0, 2 * LP, 1580, 1700},   /* and reverse: the mirror of everything is everything */
	};
	/* memchain.c:767-773 against the region [1000, 1151) x [0, 151) of a read of 151 bases: a tenth of it is 15.1 */
	static const struct { int64_t rbeg; int qbeg, len, seedlen0, want; } box[] = {
		{1010, 10, 35, 20, 1},    /* 15 > 15.1 is false */
		{1010, 10, 35, 19, 0},    /* 16 > 15.1 */
		{1010, 10, 35, 21, 1},    /* 14 */
		{1000, 0, 151, 151, 1},   /* the region itself: every edge at equality */
		{999, 10, 35, 35, 0},     /* one base before it on the reference */
		{1117, 10, 35, 35, 0},    /* ends one base after it: 1117 + 35 = 1152 */
		{1116, 10, 35, 35, 1},    /* ends with it */
		{1010, 117, 35, 35, 0},   /* ends one base after it on the read: 117 + 35 = 152 */
		{1010, 116, 35, 35, 1},
	};
	/* memchain.c:777-778, 784-785: the same region, seed (1012; 10, 35) */
	static const struct { int end, qd; int64_t rd; } dist[] = { {0, 10, 12}, {1, 106, 104} };
	/* memchain.c:779-781: min(qd, rd) asks cal_max_gap; w = min(max_gap, reg->w); qd - rd < w && rd - qd < w */
	static const struct { int qd; int64_t rd; int max_gap, rg_w, len, want; } diag[] = {
		{10, 12, 5, 100, 10, 1},
		{10, 15, 5, 100, 10, 0},     /* rd - qd == w */
		{10, 14, 5, 100, 10, 1},     /* one below */
		{15, 10, 5, 100, 10, 0},     /* qd - rd == w */
		{14, 10, 5, 100, 10, 1},
		{10, 13, 50, 3, 10, 0},      /* the region's band is the smaller: 3 */
		{10, 12, 50, 3, 10, 1},
		{106, 104, 5, 100, 104, 1},
		{4, 9, 9, 100, 4, 1},
	};
	/* memchain.c:806-813: s = (1000; 10, 21) unless stated, s_len >> 2 = 5, 95 % of 21 is 19.95 */
	static const struct { int64_t s_rbeg; int s_qbeg, s_len; int64_t t_rbeg; int t_qbeg, t_len, want; } dis[] = {
		{1000, 10, 21, 1017, 26, 20, 1},   /* overlap 31 - 26 = 5 == s_len >> 2; diagonals 16 and 17 */
		{1000, 10, 21, 1017, 26, 19, 0},   /* 19 < 19.95: too short to count */
		{1000, 10, 21, 1018, 27, 20, 0},   /* overlap 4 */
		{1000, 10, 21, 1016, 26, 20, 0},   /* the same diagonal: 16 == 16 */
		{1000, 10, 21, 989, 0, 20, 1},     /* t first: 0 + 20 - 10 = 10 >= 5; 10 != 11 */
		{1000, 10, 21, 990, 0, 20, 0},     /* the same diagonal */
		{1000, 15, 21, 984, 0, 20, 1},     /* t first, overlap 0 + 20 - 15 = 5 at equality; 15 != 16 */
		{1000, 16, 21, 983, 0, 20, 0},     /* overlap 4 */
		{1000, 10, 21, 1001, 10, 20, 1},   /* both start at the same read base */
		{1000, 10, 20, 1017, 26, 19, 0},   /* 95 % of 20 comes out as 19.0 in double, 19 < 19 is false: counted, but overlap 30 - 26 = 4 < 5 */
		{1000, 10, 20, 1016, 25, 19, 1},   /* counted, overlap 5, diagonals 15 and 16 */
		{1000, 10, 20, 1016, 25, 18, 0},   /* 18 < 19 */
	};
	/* memchain.c:623-626, 688-691 with a = 2; -7 marks a value that must stay as it was */
	static const struct { int side; int64_t rbeg; int qbeg, len, lq, want, qb; int64_t rb; int qe; int64_t re; int score, truesc; } triv[] = {
		{0, 500, 0, 30, 50, 1, 0, 500, -7, -7, 60, 60},
		{0, 500, 1, 30, 50, 0, -7, -7, -7, -7, -7, -7},
		{1, 500, 20, 30, 50, 1, -7, -7, 50, 530, -7, -7},
		{1, 500, 20, 29, 50, 0, -7, -7, -7, -7, -7, -7},
		{0, 500, 0, 50, 50, 1, 0, 500, -7, -7, 100, 100},   /* spans the read: both */
		{1, 500, 0, 50, 50, 1, -7, -7, 50, 550, -7, -7},
	};
	/* memchain.c:628-638, 654, 693-695, 713: seed (500; 10, 20) of a read of 50 at offset 1000, window [470, 560), a = 2, sc0 = 77,
	 * pen_clip5 = 5, pen_clip3 = 9 */
	static const struct { int side; uint32_t qoff; int qdir, qlen; int64_t tpos; int tdir, tlen, h0, bonus; } job[] = {
		{0, 1009, -1, 10, 499, -1, 30, 40, 5},
		{1, 1030, 1, 20, 520, 1, 40, 77, 9},
	};
	/* memchain.c:658, 717: again unless the score did not move or max_off is below three quarters of the band, aw/2 + aw/4 in shifts */
	static const struct { int score, prev, max_off, aw, want; } band[] = {
		{40, 40, 90, 100, 0},    /* score == prev, however far off the diagonal */
		{41, 40, 75, 100, 1},    /* 75 < 50 + 25 is false */
		{41, 40, 74, 100, 0},
		{41, 40, 75, 101, 1},    /* 101 >> 1 = 50, 101 >> 2 = 25 */
		{41, 40, 4, 7, 1},       /* 3 + 1 */
		{41, 40, 3, 7, 0},
	};
	/* memchain.c:662-670, 721-729: the seed of the job rows; the result has qle 8, tle 9, gtle 12; left: score 60 with pen_clip5 = 5, right:
	 * score 70 from sc0 = 40 with pen_clip3 = 9, truesc 45 before */
	static const struct { int side, score, gscore, q; int64_t r; int truesc; } settle[] = {
		{0, 60, 0, 2, 491, 60},      /* gscore == 0: local */
		{0, 60, -1, 2, 491, 60},
		{0, 60, 55, 2, 491, 60},     /* gscore == score - pen_clip5: local (with pen_clip3, 55 > 51, it would not be) */
		{0, 60, 56, 0, 488, 56},     /* one above: to the read's start */
		{0, 3, 0, 2, 491, 3},        /* score - clip < 0 == gscore: still local */
		{1, 70, 0, 38, 529, 75},     /* 45 + 70 - 40 */
		{1, 70, 61, 38, 529, 75},    /* gscore == score - pen_clip3: local */
		{1, 70, 62, 50, 532, 67},    /* one above: to the read's end, 45 + 62 - 40 (with pen_clip5 it would be local) */
	};
	/* memchain.c:265 */
	static const struct { int parent; int64_t pos; int want; } bss[] = { {0, 1000, 1}, {0, 1001, 0}, {1, 1001, 1}, {1, 1000, 0}, {0, 0, 1}, {1, 1999, 1} };
	/* memchain.c:860-863 against the region [491, 529) x [2, 38) */
	static const struct { int64_t rbeg; int qbeg, len, want; } cov[] = {
		{491, 2, 36, 1}, {491, 2, 37, 0}, {490, 2, 36, 0}, {491, 1, 36, 0}, {494, 2, 36, 0}, {493, 2, 36, 1}, {500, 10, 20, 1},
	};

	for (i = 0; i < N(span); ++i) {
		int64_t b = -7, e = -7;
		c2r_seed_span(span[i].rbeg, span[i].qbeg, span[i].len, span[i].lq, span[i].gl, span[i].gr, &b, &e);
		if (b != span[i].b || e != span[i].e) FAIL("c2r_seed_span", i);
	}
	for (i = 0; i < N(win); ++i) {
		int64_t r0 = win[i].r0, r1 = win[i].r1;
		c2r_clamp_window(&r0, &r1, LP, win[i].pos, win[i].cb, win[i].ce);
		if (r0 != win[i].x0 || r1 != win[i].x1) FAIL("c2r_clamp_window", i);
	}
	for (i = 0; i < N(box); ++i)
		if (c2r_in_box(box[i].rbeg, box[i].qbeg, box[i].len, 151, 1000, 1151, 0, 151, box[i].seedlen0) != box[i].want) FAIL("c2r_in_box", i);
	for (i = 0; i < N(dist); ++i) {
		int qd = -7; int64_t rd = -7;
		c2r_end_dist(dist[i].end, 1012, 10, 35, 1000, 1151, 0, 151, &qd, &rd);
		if (qd != dist[i].qd || rd != dist[i].rd) FAIL("c2r_end_dist", i);
	}
	for (i = 0; i < N(diag); ++i) {
		if (c2r_gap_len(diag[i].qd, diag[i].rd) != diag[i].len) FAIL("c2r_gap_len", i);
		if (c2r_near_diagonal(diag[i].qd, diag[i].rd, diag[i].max_gap, diag[i].rg_w) != diag[i].want) FAIL("c2r_near_diagonal", i);
	}
	for (i = 0; i < N(dis); ++i)
		if (c2r_disagrees(dis[i].s_rbeg, dis[i].s_qbeg, dis[i].s_len, dis[i].t_rbeg, dis[i].t_qbeg, dis[i].t_len) != dis[i].want) FAIL("c2r_disagrees", i);
	for (i = 0; i < N(triv); ++i) {
		int qb = -7, qe = -7, score = -7, truesc = -7; int64_t rb = -7, re = -7;
		if (c2r_side_trivial(triv[i].side, triv[i].rbeg, triv[i].qbeg, triv[i].len, triv[i].lq, 2, &qb, &rb, &qe, &re, &score, &truesc) != triv[i].want) FAIL("c2r_side_trivial", i);
		if (qb != triv[i].qb || rb != triv[i].rb || qe != triv[i].qe || re != triv[i].re || score != triv[i].score || truesc != triv[i].truesc) FAIL("c2r_side_trivial values", i);
	}
	for (i = 0; i < N(job); ++i) {
		const c2r_job_t j = c2r_side_job(job[i].side, 1000, 500, 10, 20, 50, 470, 560, 2, 77, 5, 9);
		if (j.qoff != job[i].qoff || j.qdir != job[i].qdir || j.qlen != job[i].qlen || j.tpos != job[i].tpos || j.tdir != job[i].tdir ||
		    j.tlen != job[i].tlen || j.h0 != job[i].h0 || j.end_bonus != job[i].bonus) FAIL("c2r_side_job", i);
	}
	for (i = 0; i < N(band); ++i)
		if (c2r_band_again(band[i].score, band[i].prev, band[i].max_off, band[i].aw) != band[i].want) FAIL("c2r_band_again", i);
	for (i = 0; i < N(settle); ++i) {
		/* the clip is the end bonus of the side's job: the pairing of side and penalty is checked with the rule */
		const c2r_job_t j = c2r_side_job(settle[i].side, 1000, 500, 10, 20, 50, 470, 560, 2, 40, 5, 9);
		int qb = -7, qe = -7, truesc = settle[i].side ? 45 : -7; int64_t rb = -7, re = -7;
		c2r_side_settle(settle[i].side, settle[i].score, 8, 9, 12, settle[i].gscore, j.end_bonus, 40, 500, 10, 20, 50, &qb, &rb, &qe, &re, &truesc);
		if (truesc != settle[i].truesc) FAIL("c2r_side_settle truesc", i);
		if (settle[i].side == 0 ? (qb != settle[i].q || rb != settle[i].r || qe != -7 || re != -7) : (qe != settle[i].q || re != settle[i].r || qb != -7 || rb != -7)) FAIL("c2r_side_settle", i);
	}
	for (i = 0; i < N(bss); ++i)
		if (c2r_bss(bss[i].parent, LP, bss[i].pos) != bss[i].want) FAIL("c2r_bss", i);
	for (i = 0; i < N(cov); ++i)
		if (c2r_covers(2, 38, 491, 529, cov[i].rbeg, cov[i].qbeg, cov[i].len) != cov[i].want) FAIL("c2r_covers", i);
	printf("ok\n");
	return 0;
}
