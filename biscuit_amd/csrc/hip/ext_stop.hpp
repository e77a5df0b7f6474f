// ext_stop.hpp -- the device forms of the stopping rule of ext_stop_rule.h (the rule and its proof are there): PHI over the layouts the extension
// kernels keep the reference's eh[] in, always in 32 bits, and the counters of the rule.
//   ext_stop_phi_reg   ext_dp_reg: lane l of slot c owns entry 64 c + l                      (ext_dp.hpp)
//   ext_stop_phi_pk    ext_dp_pk: ... entries 128 p + l and 128 p + 64 + l in the halves     (ext_pk.hpp)
//   k_ext4 and k_extl evaluate it in place over their own registers with ext_stop_term() (sixteen lanes a job; a lane a job).
// Every form evaluates PHI over exactly eh[beg .. qlen], after the band of the next row is known, on every row with m < gscore that is not the
// extension's last anyway: the row the rule fires on, and with it the number of stops, is the same whichever kernel runs the job.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_common.hpp"
#include "wave.hpp"
#include "ext_stop_rule.h"

// the counter block DevScoring::xs_ctr points to (null: nothing is counted): XS_N words per launch family
enum { XS_STOPS = 0,    // extensions the rule stopped (none with the switch off)
       XS_EVALS = 1,    // evaluations of PHI
       XS_LEFT = 2,     // rows still to run at the stop, tlen - 1 - i: an upper bound on the saving
       XS_DEAD = 3,     // with the switch off: rows actually run after the rule would have fired
       XS_WOULD = 4,    // with the switch off: extensions the rule would have stopped
       XS_N = 5 };
enum { XS_FAM_EXT4 = 0, XS_FAM_EXTL = 1, XS_FAM_TIER = 2, XS_FAM_C2R = 3, XS_FAM_WAVE = 4, XS_FAM_N = 5 };   // (WAVE: the wavefront-per-job batch form)

template <int NC>
__device__ __forceinline__ int ext_stop_phi_reg(const int (&Hr)[NC], const int (&Er)[NC], int beg, int qlen, int mx, int lane)
{
	int phi = 0;
#pragma unroll
	for (int c = 0; c < NC; ++c) {
		const int a = (c << 6) + lane;
		const int t = ext_stop_term(Hr[c], Er[c], (qlen - 1 - a) * mx, mx);
		phi = (a >= beg && a <= qlen && t > phi) ? t : phi;
	}
	return wave_max_i32(phi);
}

template <int NP, typename PK>
__device__ __forceinline__ int ext_stop_phi_pk(const PK (&Hp)[NP], const PK (&Ep)[NP], int beg, int qlen, int mx, int lane)
{
	int phi = 0;
#pragma unroll
	for (int p = 0; p < NP; ++p) {
		const uint32_t hw = __builtin_bit_cast(uint32_t, Hp[p]), ew = __builtin_bit_cast(uint32_t, Ep[p]);   // every stored half is in [0, 32767]
#pragma unroll
		for (int u = 0; u < 2; ++u) {
			const int a = (p << 7) + (u << 6) + lane;
			const int t = ext_stop_term((int)(u ? hw >> 16 : hw & 0xffffu), (int)(u ? ew >> 16 : ew & 0xffffu), (qlen - 1 - a) * mx, mx);
			phi = (a >= beg && a <= qlen && t > phi) ? t : phi;
		}
	}
	return wave_max_i32(phi);
}

// The wavefront-per-job forms, everything wave-uniform.  `fired`: the rule has fired on this extension (it goes on only with the switch off and
// the counters on, where the rows it still runs are counted).
__device__ __forceinline__ bool ext_stop_armed(const DevScoring &sc) { return sc.ext_stop != 0 || sc.xs_ctr != nullptr; }
// PHI evaluated after row i (rows_left = tlen - 1 - i > 0): counts, and says whether the extension ends here
__device__ __forceinline__ bool ext_stop_decide(const DevScoring &sc, int fam, int phi, int gscore, int rows_left, int lane, bool &fired)
{
	const bool fire = ext_stop_fires(phi, gscore);
	if (sc.xs_ctr && lane == 0) {
		unsigned long long *c = sc.xs_ctr + XS_N * fam;
		atomicAdd(&c[XS_EVALS], 1ull);
		if (fire) { atomicAdd(&c[sc.ext_stop ? XS_STOPS : XS_WOULD], 1ull); atomicAdd(&c[XS_LEFT], (unsigned long long)rows_left); }
	}
	fired = fire;
	return fire && sc.ext_stop != 0;
}
// a row begun after the rule fired (the switch off)
__device__ __forceinline__ void ext_stop_dead_row(const DevScoring &sc, int fam, int lane)
{
	if (sc.xs_ctr && lane == 0) atomicAdd(&sc.xs_ctr[XS_N * fam + XS_DEAD], 1ull);
}
