// rtw_probe.h -- what the device-math probe (rtw_probe.hip, rtw.h "device math, for tests") shares between host and device: the exact
// rounding predicates, the operand generators of the in-kernel sweeps, and the two calls the shim forwards to.  Integer code only: the
// predicates decide "is this the correctly rounded f32 result" without trusting any floating-point unit, so the same text is the reference on
// the GPU (inside the sweep kernels) and on the host (rtw_rounding_check, which the CPU tests hold against Python's big integers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rtw.h"

namespace rtw {

// ---- a normal, finite f32 as sign, 24-bit mantissa (hidden bit set) and unbiased exponent: |v| = m * 2^(e - 23) ---------------------------
struct F32Parts { uint32_t neg, m; int32_t e; bool normal; };
__host__ __device__ __forceinline__ F32Parts f32_parts(uint32_t bits) {
    F32Parts p;
    const uint32_t be = (bits >> 23) & 0xFFu;
    p.neg = bits >> 31;
    p.m = (bits & 0x007FFFFFu) | 0x00800000u;
    p.e = (int32_t)be - 127;
    p.normal = be != 0u && be != 0xFFu;
    return p;
}
// The two half-way neighbours of the f32 m * 2^(e - 23), in quarter ulps: lo = 4m - 2 and hi = 4m + 2, except that directly above a power of
// two the f32 below is half an ulp away, so the half-way point is a QUARTER ulp down (lo = 4m - 1) -- unless that power is 2^-126, below which
// the subnormals keep the spacing.  Above 0xFFFFFF * 2^(e - 23) the next f32 is one ulp up whether or not it is finite (IEEE rounds as if the
// exponent range were unbounded, then overflows).
__host__ __device__ __forceinline__ void f32_halfway(uint32_t m, int32_t e, uint64_t &lo, uint64_t &hi) {
    lo = 4ull * m - ((m == 0x00800000u && e > -126) ? 1ull : 2ull);
    hi = 4ull * m + 2ull;
}

// Is `s` the correctly rounded f32 sqrt of the positive normal f32 `x` (both as bit patterns)?  x lies strictly between the squares of s's
// half-way neighbours (a square of a half-way point has 50 significant bits: no ties).  With x = mx 2^(ex - 23) and the neighbours
// L 2^(es - 25):  L^2 2^(2 es - 50) < mx 2^(ex - 23)  <=>  L^2 < mx 2^(ex - 2 es + 27); L < 2^26, so both sides are below 2^53 for any shift that a
// right answer can have (27 or 28, 26 when s rounded up into the next binade); any other shift is a wrong s.
__host__ __device__ __forceinline__ bool sqrt_is_rounded(uint32_t x_bits, uint32_t s_bits) {
    const F32Parts x = f32_parts(x_bits), s = f32_parts(s_bits);
    if (!x.normal || x.neg || !s.normal || s.neg) return false;
    const int32_t sh = x.e - 2 * s.e + 27;
    if (sh < 20 || sh > 34) return false;
    uint64_t lo, hi;
    f32_halfway(s.m, s.e, lo, hi);
    const uint64_t v = (uint64_t)x.m << sh;
    return lo * lo < v && v < hi * hi;
}
// Is `q` the correctly rounded f32 n / d for normal f32 n (or a zero), d and q?  |n| lies strictly between |d| times q's half-way neighbours (d
// times a half-way point has 25 significant bits at least: no ties while q is normal), and the sign is the operands'.  With the neighbours
// L 2^(eq - 25):  md L 2^(ed + eq - 48) < mn 2^(en - 23)  <=>  md L < mn 2^(en - ed - eq + 25);  md L < 2^50, and a right answer has a shift of 25 or 26.
// n = +-0: q is the zero of that sign.
__host__ __device__ __forceinline__ bool div_is_rounded(uint32_t n_bits, uint32_t d_bits, uint32_t q_bits) {
    const F32Parts n = f32_parts(n_bits), d = f32_parts(d_bits), q = f32_parts(q_bits);
    if (!d.normal) return false;
    if ((n.neg ^ d.neg) != q.neg) return false;
    if ((n_bits & 0x7FFFFFFFu) == 0u) return (q_bits & 0x7FFFFFFFu) == 0u;
    if (!n.normal || !q.normal) return false;
    const int32_t sh = n.e - d.e - q.e + 25;
    if (sh < 20 || sh > 34) return false;
    uint64_t lo, hi;
    f32_halfway(q.m, q.e, lo, hi);
    const uint64_t v = (uint64_t)n.m << sh;
    return (uint64_t)d.m * lo < v && v < (uint64_t)d.m * hi;
}

// ---- operands of the in-kernel sweeps, from the global index alone ---------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint32_t probe_mix32(uint32_t x) {           // lowbias32, as mix32 (rtw_device.h)
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
// draw k of pair `index` under `seed`: a counter hash, chained like the render's streams
__host__ __device__ __forceinline__ uint32_t probe_draw(uint32_t seed, uint64_t index, uint32_t k) {
    uint32_t h = probe_mix32(seed + 0x9E3779B9U);
    h = probe_mix32(h ^ (uint32_t)(index >> 32));
    h = probe_mix32(h ^ (uint32_t)index);
    return probe_mix32(h ^ (0x85EBCA6BU * (k + 1u)));
}
__host__ __device__ __forceinline__ uint32_t probe_f32_bits(uint32_t neg, uint32_t m24, int32_t e) {
    return (neg << 31) | ((uint32_t)(e + 127) << 23) | (m24 & 0x007FFFFFu);
}
// Signs and exponents of a pair: independent signs, d's exponent uniform over [-40, 39] and n's over [-60, 39] -- with any mantissa that is
// |d| in [2^-40, 2^40) and |n| in [2^-60, 2^40); the closed ends themselves are single values, tested element-wise.
__host__ __device__ __forceinline__ void probe_pair_frame(uint32_t r, uint32_t &neg_n, uint32_t &neg_d, int32_t &en, int32_t &ed) {
    neg_n = r & 1u; neg_d = (r >> 1) & 1u;
    ed = -40 + (int32_t)((((r >> 2) & 0x7FFFu) * 80u) >> 15);
    en = -60 + (int32_t)((((r >> 17) & 0x7FFFu) * 100u) >> 15);
}
// RTW_SWEEP_DIV_RANDOM: 24-bit mantissas from two draws
__host__ __device__ __forceinline__ void probe_div_random(uint32_t seed, uint64_t index, uint32_t &n_bits, uint32_t &d_bits) {
    uint32_t neg_n, neg_d; int32_t en, ed;
    probe_pair_frame(probe_draw(seed, index, 0), neg_n, neg_d, en, ed);
    n_bits = probe_f32_bits(neg_n, 0x00800000u | (probe_draw(seed, index, 1) & 0x007FFFFFu), en);
    d_bits = probe_f32_bits(neg_d, 0x00800000u | (probe_draw(seed, index, 2) & 0x007FFFFFu), ed);
}
// RTW_SWEEP_DIV_MIDPOINT: quotients as close to a rounding boundary as f32 operands allow.  A boundary between two quotient mantissas is c / 2
// for an odd 25-bit c; n / d sits next to it when mn 2^k is next to c md, and since c md is odd the closest an integer multiple of 2^k comes
// is c md -+ 1.  So for an odd mantissa md (a draw) c is the odd 25-bit integer with c md = +-1 (mod 2^k) -- its low bits are md's inverse
// modulo 2^k, or minus that -- and mn = (c md -+ 1) / 2^k, the integer nearest to c md / 2^k, with k = 24 or 25 so that it has 24 bits.  The
// exact quotient is then 1 / (2 md) < 2^-24 of an ulp below (or above) the boundary.  A draw asks for one side; of the two residues modulo 2^25
// exactly one has bit 24 set, and where the asked one has not and c = 2^24 + residue would make mn a 25-bit number, the other side is taken.
__host__ __device__ __forceinline__ void probe_midpoint_mantissas(uint32_t r_md, uint32_t want_above, uint32_t &mn, uint32_t &md, uint32_t &c,
                                                                  uint32_t &k, uint32_t &above) {
    md = 0x00800000u | (r_md & 0x007FFFFFu) | 1u;
    uint32_t inv = md;                                                  // md * md = 1 (mod 8); each step doubles the correct bits
    inv *= 2u - md * inv; inv *= 2u - md * inv; inv *= 2u - md * inv; inv *= 2u - md * inv;
    inv &= 0x01FFFFFFu;                                                 // md * inv = 1 (mod 2^25)
    above = want_above & 1u;
    uint32_t res = above ? (0x02000000u - inv) : inv;                   // c md = -1: n / d is above the boundary;  = +1: below
    if (res < 0x01000000u && ((uint64_t)(res | 0x01000000u) * md) >= (1ull << 48)) { above ^= 1u; res = 0x02000000u - res; }
    c = res | 0x01000000u;
    const uint64_t p = (uint64_t)c * md;
    k = p >= (1ull << 48) ? 25u : 24u;
    mn = (uint32_t)((above ? p + 1ull : p - 1ull) >> k);
}
__host__ __device__ __forceinline__ void probe_div_midpoint(uint32_t seed, uint64_t index, uint32_t &n_bits, uint32_t &d_bits) {
    uint32_t neg_n, neg_d, mn, md, c, k, above; int32_t en, ed;
    const uint32_t r0 = probe_draw(seed, index, 0);
    probe_pair_frame(r0, neg_n, neg_d, en, ed);
    probe_midpoint_mantissas(probe_draw(seed, index, 1), probe_draw(seed, index, 2), mn, md, c, k, above);
    n_bits = probe_f32_bits(neg_n, mn, en);
    d_bits = probe_f32_bits(neg_d, md, ed);
}

// ---- the calls behind rtw_ctx_device_math / rtw_ctx_device_sweep (rtw_shim.hip owns the context and has checked it) ---------------------------
// columns a function reads and writes, 0 for an unknown fn
void device_math_cols(uint32_t fn, uint32_t &in_cols, uint32_t &out_cols);
int device_math_device(int device, hipStream_t stream, uint32_t fn, const float *in, uint32_t n_cols, uint32_t n, float *out, uint32_t out_cols,
                       int *last_hip);
int device_sweep_device(int device, hipStream_t stream, uint32_t which, uint64_t first, uint64_t count, uint32_t seed, RtwSweepResult *result,
                        int *last_hip);

} // namespace rtw
