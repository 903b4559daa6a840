// rtw_filter.hip -- Rust2's bilateral post-process (Rust2/src/postprocessing.rs:12-131) on the host and on the GPU, bit for bit.
//
// The reference (per output pixel, f32, libm expf):
//   spatial  = ceil(0.02 * sqrt((w*w + h*h) as f32));          inv_spatial = 0.5 / (spatial * spatial)
//   gradient = serial sum over y in 1..h-1, x in 1..w-1 of sqrt((Iu-Id)^2 + (Il-Ir)^2)
//   avg      = gradient / ((w-2)*(h-2)) as f32;                 inv_range   = 0.5 / (avg * avg)
//   for (xi, yi) in the window (column outer, row inner), for each channel c, k = pi[c] - p[c]:
//     w = exp((-inv_spatial) * (dx*dx + dy*dy) as f32 - inv_range * (k as f32 / 255)^2)
//     col_sum[c] += pi[c] as f32 * w / 255;  w_sum[c] += w
//   out[c] = (col_sum[c] * 255 / w_sum[c]) as u8
// The weight depends on (d2 = dx*dx + dy*dy, |k|) only.  Once the range term is known the host evaluates libm expf for every d2 the
// window can produce and every |k| in 0..255 (one row of 256 floats per distinct d2, reached through a d2 -> row map); the device only
// looks weights up, so its weights are the host's bit for bit.  One thread per output pixel keeps the reference's summation order.
// The gradient sum is an f32 sum of ~2 M terms whose association fixes `avg`: it is added in the reference's order, by one wave.
// Everything here is compiled with -ffp-contract=off and correctly rounded f32 division and sqrt (Makefile), like the reference.
#include "rtw_filter.h"
#include "rtw_devmem.h"
#include "rtw_exp.h"
#include "rtw_host.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

namespace rtw {
namespace {

constexpr uint32_t FBX = 32, FBY = 16;          // filter workgroup: 32 x 16 output pixels (a wave covers two rows of 32: conflict-free tile reads)
constexpr uint32_t SUM_CHUNK = 2048;            // terms the summing wave moves through LDS per step: 8 float4 per lane
constexpr uint32_t TABLE_LDS_MAX = 80u * 1024u; // table + tile in LDS while two workgroups still fit in a CU's 160 KiB; else the table stays global
// The guided filter (profiles/guided_lds_ab.log): the guide planes sit in LDS behind the pixel tile while both fit in
// GUIDED_GUIDE_LDS_MAX, else the taps' guides are read from global memory; the table joins them only while everything still fits in
// GUIDED_TABLE_LDS_MAX (two workgroups per CU) -- at 1080p / size 10 the table in global memory beside guides in LDS was the fastest.
constexpr uint32_t GUIDED_GUIDE_LDS_MAX = 80u * 1024u;
constexpr uint32_t GUIDED_TABLE_LDS_MAX = 80u * 1024u;
constexpr uint32_t GUIDED_LDS_CAP = 160u * 1024u;         // what a workgroup can have at all: the limit of an RTW_OPT_GUIDED_LAYOUT request

// ---- the arithmetic shared by the host path and the kernels ------------------------------------------------------------------------
// intensity (postprocessing.rs:64-68): 0.2989 * r / 255 + 0.5870 * g / 255 + 0.1140 * b / 255, left to right
__host__ __device__ inline float intensity(const uint8_t *p) {
    return (0.2989f * (float)p[0]) / 255.0f + (0.5870f * (float)p[1]) / 255.0f + (0.1140f * (float)p[2]) / 255.0f;
}

// the gradient term of interior pixel (x, y) (postprocessing.rs:76-83)
__host__ __device__ inline float gradient_term(const uint8_t *img, uint32_t w, uint32_t x, uint32_t y) {
    const float iu = intensity(img + 3 * ((size_t)(y - 1) * w + x));
    const float id = intensity(img + 3 * ((size_t)(y + 1) * w + x));
    const float ir = intensity(img + 3 * ((size_t)y * w + x + 1));
    const float il = intensity(img + 3 * ((size_t)y * w + x - 1));
    return sqrtf((iu - id) * (iu - id) + (il - ir) * (il - ir));
}

// Rust `f as u8`: truncate, saturate to [0, 255], NaN -> 0
__host__ __device__ inline uint8_t rust_as_u8(float v) {
    if (!(v > 0.0f)) return 0;
    if (v >= 255.0f) return 255;
    return (uint8_t)v;
}

// Rust2 Vec3::to_rgb_u8 (as rtw_quantize_u8_rust2)
__host__ __device__ inline uint8_t quantize_rust2(float c) {
    float v = c * 255.99f;
    v = v != v ? v : (v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v));
    v = roundf(v);
    return v != v ? 0 : (uint8_t)v;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bilateral_quantize_kernel(const float *__restrict__ in, size_t n, uint8_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = quantize_rust2(in[i]);
}

// terms[(y-1)*(w-2) + (x-1)] for the interior pixels, in the order the reference adds them
__global__ void __launch_bounds__(256) bilateral_gradient_terms_kernel(const uint8_t *__restrict__ img, uint32_t w, uint32_t n,
                                                                       float *__restrict__ terms) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t iw = w - 2;
    terms[i] = gradient_term(img, w, 1 + i % iw, 1 + i / iw);
}

// The serial sum, by ONE wave: it streams SUM_CHUNK terms per step from global memory into LDS (the next step's loads are in flight while
// it adds the current one) and every lane runs the same dependent chain of f32 adds over the LDS copy (uniform addresses: broadcast reads).
// Past the end the loads give +0.0f, which leaves the sum unchanged (s + 0 == s for every s the chain can hold: it starts at +0 and the
// terms are square roots, never negative).
__global__ void __launch_bounds__(64) bilateral_gradient_sum_kernel(const float *__restrict__ terms, uint32_t n, float *__restrict__ out) {
    __shared__ float4 buf[2][SUM_CHUNK / 4];
    const uint32_t lane = threadIdx.x;
    const uint32_t n_chunks = (n + SUM_CHUNK - 1) / SUM_CHUNK;
    float4 r[8];
    auto fetch = [&](uint32_t chunk) {
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const uint32_t i = chunk * SUM_CHUNK + 4 * (k * 64 + lane);
            if (i + 3 < n) r[k] = *(const float4 *)(terms + i);
            else {
                r[k].x = i < n ? terms[i] : 0.0f;
                r[k].y = i + 1 < n ? terms[i + 1] : 0.0f;
                r[k].z = i + 2 < n ? terms[i + 2] : 0.0f;
                r[k].w = 0.0f;
            }
        }
    };
    auto stash = [&](uint32_t slot) {
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) buf[slot][k * 64 + lane] = r[k];
    };
    fetch(0);
    stash(0);
    __syncthreads();
    float s = 0.0f;
    for (uint32_t c = 0; c < n_chunks; c++) {
        const bool more = c + 1 < n_chunks;
        if (more) fetch(c + 1);
        const float4 *b = buf[c & 1];
#pragma unroll 16
        for (uint32_t j = 0; j < SUM_CHUNK / 4; j++) {
            const float4 v = b[j];
            s += v.x;
            s += v.y;
            s += v.z;
            s += v.w;
        }
        if (more) stash((c + 1) & 1);
        __syncthreads();
    }
    if (lane == 0) *out = s;
}

// One thread per output pixel.  The workgroup's pixels plus a halo of `s` (packed r | g << 8 | b << 16) and, with TABLE_LDS, the weight
// table sit in LDS.  Every thread runs the same (dx, dy) loop -- column outer, row inner, the window of an interior pixel -- so the d2 -> row
// lookup is uniform; a tap outside the thread's own (clipped, asymmetric) window is skipped, which keeps the taps it takes in the reference's
// order.  Edges bounds the inner loop to |dx| + |dy| < s.
template <bool TABLE_LDS>
__global__ void __launch_bounds__(FBX * FBY) bilateral_filter_kernel(const uint8_t *__restrict__ img, uint32_t w, uint32_t h, int s, int edges,
                                                                     const float *__restrict__ table, uint32_t table_floats,
                                                                     const uint16_t *__restrict__ rowmap, uint8_t *__restrict__ out) {
    extern __shared__ uint32_t smem[];
    float *ltab = (float *)smem;
    uint32_t *tile = smem + (TABLE_LDS ? table_floats : 0);
    const int tx = (int)(threadIdx.x % FBX), ty = (int)(threadIdx.x / FBX);
    const int x0 = (int)(blockIdx.x * FBX), y0 = (int)(blockIdx.y * FBY);
    const int tw = (int)FBX + 2 * s, th = (int)FBY + 2 * s;          // the tile covers x0 - s .. x0 + FBX + s, y0 - s .. y0 + FBY + s
    for (int i = (int)threadIdx.x; i < tw * th; i += (int)(FBX * FBY)) {
        const int ix = x0 - s + i % tw, iy = y0 - s + i / tw;
        uint32_t v = 0;
        if (ix >= 0 && iy >= 0 && ix < (int)w && iy < (int)h) {
            const uint8_t *p = img + 3 * ((size_t)iy * w + ix);
            v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        }
        tile[i] = v;
    }
    if (TABLE_LDS)
        for (uint32_t i = threadIdx.x; i < table_floats / 4; i += FBX * FBY) ((float4 *)ltab)[i] = ((const float4 *)table)[i];
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x >= (int)w || y >= (int)h) return;
    const uint32_t pc = tile[(ty + s) * tw + tx + s];
    const int p0 = (int)(pc & 255u), p1 = (int)((pc >> 8) & 255u), p2 = (int)(pc >> 16);
    // the window (postprocessing.rs:30-35) as offsets: dx in [-min(x, s), min(w-x-1, s)), dy likewise
    const int lx = -min(x, s), hx = min((int)w - x - 1, s), ly = -min(y, s), hy = min((int)h - y - 1, s);
    float cs0 = 0.0f, cs1 = 0.0f, cs2 = 0.0f, ws0 = 0.0f, ws1 = 0.0f, ws2 = 0.0f;
    for (int dx = -s; dx < s; dx++) {
        const int adx = dx < 0 ? -dx : dx;
        const int dy_lo = edges ? -(s - 1 - adx) : -s, dy_hi = edges ? s - 1 - adx : s - 1;     // inclusive
        const bool col_in = dx >= lx && dx < hx;
        const uint32_t *trow = tile + (ty + s) * tw + tx + s + dx;
        for (int dy = dy_lo; dy <= dy_hi; dy++) {
            const float *t = (TABLE_LDS ? ltab : table) + 256u * rowmap[dx * dx + dy * dy];
            if (col_in && dy >= ly && dy < hy) {
                const uint32_t q = trow[dy * tw];
                const int q0 = (int)(q & 255u), q1 = (int)((q >> 8) & 255u), q2 = (int)(q >> 16);
                const float w0 = t[q0 > p0 ? q0 - p0 : p0 - q0], w1 = t[q1 > p1 ? q1 - p1 : p1 - q1], w2 = t[q2 > p2 ? q2 - p2 : p2 - q2];
                cs0 += ((float)q0 * w0) / 255.0f; ws0 += w0;
                cs1 += ((float)q1 * w1) / 255.0f; ws1 += w1;
                cs2 += ((float)q2 * w2) / 255.0f; ws2 += w2;
            }
        }
    }
    uint8_t *o = out + 3 * ((size_t)y * w + x);
    o[0] = rust_as_u8((cs0 * 255.0f) / ws0);
    o[1] = rust_as_u8((cs1 * 255.0f) / ws1);
    o[2] = rust_as_u8((cs2 * 255.0f) / ws2);
}

// ---- the guided (joint bilateral) filter: DESIGN.md 8b -----------------------------------------------------------------------------
// The guide weight of tap q for centre p, one definition for the host path and the kernel.  TERMS: GUIDE_DEPTH | GUIDE_NORMAL | GUIDE_IDX.
//   a = 0;  depth: a += inv_depth * dz^2;  normal: a += inv_normal * ((dx^2 + dy^2) + dz^2);  g = a >= 0 ? exp_plain(-a) : 0 (a NaN a drops
//   the tap);  same_object: g = 0 where the ids differ.
constexpr int GUIDE_DEPTH = 1, GUIDE_NORMAL = 2, GUIDE_IDX = 4;

struct GuidePixel { float z, nx, ny, nz; int32_t id; };

template <int TERMS>
__host__ __device__ inline float guide_weight(float inv_depth, float inv_normal, const GuidePixel &p, const GuidePixel &q) {
    float a = 0.0f;
    if (TERMS & GUIDE_DEPTH) {
        const float dz = q.z - p.z;
        a = a + inv_depth * (dz * dz);
    }
    if (TERMS & GUIDE_NORMAL) {
        const float dx = q.nx - p.nx, dy = q.ny - p.ny, dz = q.nz - p.nz;
        a = a + inv_normal * ((dx * dx + dy * dy) + dz * dz);
    }
    float g = a >= 0.0f ? exp_plain(-a) : 0.0f;
    if ((TERMS & GUIDE_IDX) && q.id != p.id) g = 0.0f;
    return g;
}

// pixel i of the guide planes ([h][w] f32, [h][w][3] f32, [h][w] i32); a plane whose term is off is not read
template <int TERMS>
__host__ __device__ inline GuidePixel guide_load(const float *depth, const float *normal, const int32_t *idx, size_t i) {
    GuidePixel g = { 0.0f, 0.0f, 0.0f, 0.0f, 0 };
    if (TERMS & GUIDE_DEPTH) g.z = depth[i];
    if (TERMS & GUIDE_NORMAL) { g.nx = normal[3 * i]; g.ny = normal[3 * i + 1]; g.nz = normal[3 * i + 2]; }
    if (TERMS & GUIDE_IDX) g.id = idx[i];
    return g;
}

constexpr uint32_t guide_planes(int terms) { return (terms & GUIDE_DEPTH ? 1u : 0u) + (terms & GUIDE_NORMAL ? 3u : 0u) + (terms & GUIDE_IDX ? 1u : 0u); }

// bilateral_filter_kernel with every tap's three weights multiplied by the guide weight: the same workgroup, tile, loop and tap order.
// LDS (dwords): [table, with TABLE_LDS][packed-pixel tile][with GUIDE_LDS one plane of tile size per guide component: z | nx | ny | nz | id].
// The planes are separate arrays, so a wave's read of one component is two rows of 32 consecutive dwords like the pixel tile's.  Without
// GUIDE_LDS the taps' guides come from global memory (a wave reads two runs of 32 consecutive pixels per plane).  TERMS == 0 is the plain
// filter: no guide is touched and no weight is multiplied.
template <bool TABLE_LDS, bool GUIDE_LDS, int TERMS>
__global__ void __launch_bounds__(FBX * FBY) guided_filter_kernel(const uint8_t *__restrict__ img, uint32_t w, uint32_t h, int s, int edges,
                                                                  const float *__restrict__ table, uint32_t table_floats,
                                                                  const uint16_t *__restrict__ rowmap, const float *__restrict__ depth,
                                                                  const float *__restrict__ normal, const int32_t *__restrict__ idx,
                                                                  float inv_depth, float inv_normal, uint8_t *__restrict__ out) {
    extern __shared__ uint32_t smem[];
    float *ltab = (float *)smem;
    uint32_t *tile = smem + (TABLE_LDS ? table_floats : 0);
    const int tx = (int)(threadIdx.x % FBX), ty = (int)(threadIdx.x / FBX);
    const int x0 = (int)(blockIdx.x * FBX), y0 = (int)(blockIdx.y * FBY);
    const int tw = (int)FBX + 2 * s, th = (int)FBY + 2 * s;
    const int tn = tw * th;
    // the guide planes behind the tile, in the order z, nx, ny, nz, id; an absent one takes no room
    float *gz = (float *)(tile + tn);
    float *gn = gz + ((TERMS & GUIDE_DEPTH) ? tn : 0);
    int32_t *gi = (int32_t *)(gn + ((TERMS & GUIDE_NORMAL) ? 3 * tn : 0));
    for (int i = (int)threadIdx.x; i < tn; i += (int)(FBX * FBY)) {
        const int ix = x0 - s + i % tw, iy = y0 - s + i / tw;
        const bool in = ix >= 0 && iy >= 0 && ix < (int)w && iy < (int)h;
        uint32_t v = 0;
        if (in) {
            const uint8_t *p = img + 3 * ((size_t)iy * w + ix);
            v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        }
        tile[i] = v;
        if (GUIDE_LDS && TERMS) {
            GuidePixel g = { 0.0f, 0.0f, 0.0f, 0.0f, 0 };
            if (in) g = guide_load<TERMS>(depth, normal, idx, (size_t)iy * w + ix);
            if (TERMS & GUIDE_DEPTH) gz[i] = g.z;
            if (TERMS & GUIDE_NORMAL) { gn[i] = g.nx; gn[tn + i] = g.ny; gn[2 * tn + i] = g.nz; }
            if (TERMS & GUIDE_IDX) gi[i] = g.id;
        }
    }
    if (TABLE_LDS)
        for (uint32_t i = threadIdx.x; i < table_floats / 4; i += FBX * FBY) ((float4 *)ltab)[i] = ((const float4 *)table)[i];
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x >= (int)w || y >= (int)h) return;
    const int centre = (ty + s) * tw + tx + s;
    const uint32_t pc = tile[centre];
    const int p0 = (int)(pc & 255u), p1 = (int)((pc >> 8) & 255u), p2 = (int)(pc >> 16);
    const size_t pix = (size_t)y * w + x;
    const GuidePixel gp = guide_load<TERMS>(depth, normal, idx, pix);
    const int lx = -min(x, s), hx = min((int)w - x - 1, s), ly = -min(y, s), hy = min((int)h - y - 1, s);
    float cs0 = 0.0f, cs1 = 0.0f, cs2 = 0.0f, ws0 = 0.0f, ws1 = 0.0f, ws2 = 0.0f;
    for (int dx = -s; dx < s; dx++) {
        const int adx = dx < 0 ? -dx : dx;
        const int dy_lo = edges ? -(s - 1 - adx) : -s, dy_hi = edges ? s - 1 - adx : s - 1;     // inclusive
        const bool col_in = dx >= lx && dx < hx;
        for (int dy = dy_lo; dy <= dy_hi; dy++) {
            const float *t = (TABLE_LDS ? ltab : table) + 256u * rowmap[dx * dx + dy * dy];
            if (col_in && dy >= ly && dy < hy) {
                const int off = centre + dy * tw + dx;
                const uint32_t q = tile[off];
                const int q0 = (int)(q & 255u), q1 = (int)((q >> 8) & 255u), q2 = (int)(q >> 16);
                float w0 = t[q0 > p0 ? q0 - p0 : p0 - q0], w1 = t[q1 > p1 ? q1 - p1 : p1 - q1], w2 = t[q2 > p2 ? q2 - p2 : p2 - q2];
                if (TERMS) {
                    GuidePixel gq = { 0.0f, 0.0f, 0.0f, 0.0f, 0 };
                    if (GUIDE_LDS) {
                        if (TERMS & GUIDE_DEPTH) gq.z = gz[off];
                        if (TERMS & GUIDE_NORMAL) { gq.nx = gn[off]; gq.ny = gn[tn + off]; gq.nz = gn[2 * tn + off]; }
                        if (TERMS & GUIDE_IDX) gq.id = gi[off];
                    } else {
                        gq = guide_load<TERMS>(depth, normal, idx, (size_t)((int64_t)pix + (int64_t)dy * (int64_t)w + dx));
                    }
                    const float g = guide_weight<TERMS>(inv_depth, inv_normal, gp, gq);
                    w0 = w0 * g; w1 = w1 * g; w2 = w2 * g;
                }
                cs0 += ((float)q0 * w0) / 255.0f; ws0 += w0;
                cs1 += ((float)q1 * w1) / 255.0f; ws1 += w1;
                cs2 += ((float)q2 * w2) / 255.0f; ws2 += w2;
            }
        }
    }
    uint8_t *o = out + 3 * pix;
    o[0] = rust_as_u8((cs0 * 255.0f) / ws0);
    o[1] = rust_as_u8((cs1 * 255.0f) / ws1);
    o[2] = rust_as_u8((cs2 * 255.0f) / ws2);
}

// ---- host side: checks, the window's d2 rows, the weight table ---------------------------------------------------------------------
int check_args(const void *in, uint32_t w, uint32_t h, const RtwBilateral *p, const uint8_t *out) {
    if (!in || !p || !out) return RTW_E_INVALID;
    if (w < 3 || h < 3) return RTW_E_INVALID;                                        // (w-2)*(h-2): the reference panics
    if ((uint64_t)w * w + (uint64_t)h * h > 0xFFFFFFFFull) return RTW_E_INVALID;     // w*w + h*h is u32 there
    if (p->proximity > RTW_PROXIMITY_EDGES || p->in_format > RTW_PIXELS_F32_RUST2) return RTW_E_INVALID;
    if (p->size > RTW_BILATERAL_MAX_SIZE) return RTW_E_INVALID;
    if (!(p->avg_gradient >= 0.0f) || !std::isfinite(p->avg_gradient)) return RTW_E_INVALID;
    return RTW_OK;
}

struct Plan {
    float spatial = 0.0f, inv_spatial = 0.0f;
    std::vector<uint16_t> rowmap;   // [2 s^2 + 1]: d2 -> table row (rows in increasing d2)
    std::vector<uint32_t> row_d2;   // [n_rows]
    uint64_t taps = 0;
};

// The (dx, dy) offsets of an interior window, as the kernel walks them: dx in [-s, s), dy in [-s, s) (Square) or |dx| + |dy| < s (Edges)
template <class F>
void for_offsets(int s, bool edges, F f) {
    for (int dx = -s; dx < s; dx++) {
        const int adx = dx < 0 ? -dx : dx;
        const int lo = edges ? -(s - 1 - adx) : -s, hi = edges ? s - 1 - adx : s - 1;
        for (int dy = lo; dy <= hi; dy++) f(dx, dy);
    }
}

// pixels of a row of length n whose window takes offset d
uint64_t offset_count(int d, int s, uint32_t n) {
    if (d >= 0) return d < s && (int64_t)n - 1 - d > 0 ? (uint64_t)((int64_t)n - 1 - d) : 0;
    return -d <= s && (int64_t)n + d > 0 ? (uint64_t)((int64_t)n + d) : 0;
}

void make_plan(uint32_t w, uint32_t h, uint32_t size, bool edges, Plan &pl) {
    pl.spatial = std::ceil(0.02f * std::sqrt((float)(w * w + h * h)));
    pl.inv_spatial = 0.5f / (pl.spatial * pl.spatial);
    const int s = (int)size;
    std::vector<uint8_t> used(2 * (size_t)s * s + 1, 0);
    pl.taps = 0;
    for_offsets(s, edges, [&](int dx, int dy) {
        used[dx * dx + dy * dy] = 1;
        pl.taps += offset_count(dx, s, w) * offset_count(dy, s, h);    // the window is a product of a column range and a row range
    });
    pl.rowmap.assign(used.size(), 0);
    pl.row_d2.clear();
    for (size_t d2 = 0; d2 < used.size(); d2++)
        if (used[d2]) { pl.rowmap[d2] = (uint16_t)pl.row_d2.size(); pl.row_d2.push_back((uint32_t)d2); }
}

float range_term(float avg) { return 0.5f / (avg * avg); }

// table[row][|k|] = expf((-inv_spatial) * d2 - inv_range * (|k| / 255)^2) with the platform's libm, as Rust's f32::exp
void build_table(const Plan &pl, float inv_range, float *table) {
    for (size_t r = 0; r < pl.row_d2.size(); r++) {
        const float a = (-pl.inv_spatial) * (float)pl.row_d2[r];
        for (int k = 0; k < 256; k++) {
            const float t = (float)k / 255.0f;
            const float b = inv_range * (t * t);
            table[r * 256 + k] = expf(a - b);
        }
    }
}

// the reference's serial gradient sum
float host_gradient_sum(const uint8_t *img, uint32_t w, uint32_t h) {
    float sum = 0.0f;
    for (uint32_t y = 1; y < h - 1; y++)
        for (uint32_t x = 1; x < w - 1; x++) sum += gradient_term(img, w, x, y);
    return sum;
}

float avg_from_sum(float sum, uint32_t w, uint32_t h) { return sum / (float)((w - 2) * (h - 2)); }

// rows [y_begin, y_end) of the filter, in the reference's form (postprocessing.rs:95-128)
void host_filter_rows(const uint8_t *img, uint32_t w, uint32_t h, uint32_t size, bool edges, const Plan &pl, const float *table,
                      uint8_t *out, uint32_t y_begin, uint32_t y_end) {
    for (uint32_t y = y_begin; y < y_end; y++)
        for (uint32_t x = 0; x < w; x++) {
            const uint8_t *p = img + 3 * ((size_t)y * w + x);
            const uint32_t left = x - std::min(x, size), right = x + std::min(w - x - 1, size);
            const uint32_t up = y - std::min(y, size), down = y + std::min(h - y - 1, size);
            float col[3] = { 0, 0, 0 }, ws[3] = { 0, 0, 0 };
            for (uint32_t xi = left; xi < right; xi++)
                for (uint32_t yi = up; yi < down; yi++) {
                    const int dx = (int)xi - (int)x, dy = (int)yi - (int)y;
                    if (edges && !((uint32_t)(std::abs(dx) + std::abs(dy)) < size)) continue;
                    const float *t = table + 256u * pl.rowmap[dx * dx + dy * dy];
                    const uint8_t *q = img + 3 * ((size_t)yi * w + xi);
                    for (int c = 0; c < 3; c++) {
                        const float wt = t[std::abs((int)q[c] - (int)p[c])];
                        col[c] += ((float)q[c] * wt) / 255.0f;
                        ws[c] += wt;
                    }
                }
            for (int c = 0; c < 3; c++) out[3 * ((size_t)y * w + x) + c] = rust_as_u8((col[c] * 255.0f) / ws[c]);
        }
}

// ---- the guided filter on the host ---------------------------------------------------------------------------------------------------
struct GuideArgs {
    const float *depth = nullptr, *normal = nullptr;
    const int32_t *idx = nullptr;
    float inv_depth = 0.0f, inv_normal = 0.0f;
    int terms = 0;                                 // GUIDE_DEPTH | GUIDE_NORMAL | GUIDE_IDX: the terms that are on
};

// everything rtw_bilateral_filter refuses, and the guide terms (rtw.h); fills `g` (a guide whose term is off is dropped here: never read)
int check_guided_args(const void *in, uint32_t w, uint32_t h, const float *depth, const float *normal, const int32_t *idx,
                      const RtwGuidedFilter *p, const uint8_t *out, GuideArgs &g) {
    if (!p) return RTW_E_INVALID;
    const int rc = check_args(in, w, h, &p->base, out);
    if (rc != RTW_OK) return rc;
    if (!(p->sigma_depth >= 0.0f) || !std::isfinite(p->sigma_depth)) return RTW_E_INVALID;
    if (!(p->sigma_normal >= 0.0f) || !std::isfinite(p->sigma_normal)) return RTW_E_INVALID;
    if (p->same_object > 1) return RTW_E_INVALID;
    g = GuideArgs();
    if (p->sigma_depth > 0.0f) {
        g.inv_depth = 0.5f / (p->sigma_depth * p->sigma_depth);
        if (!depth || !std::isfinite(g.inv_depth)) return RTW_E_INVALID;        // (a tiny sigma: inf * 0 for equal guides)
        g.depth = depth;
        g.terms |= GUIDE_DEPTH;
    }
    if (p->sigma_normal > 0.0f) {
        g.inv_normal = 0.5f / (p->sigma_normal * p->sigma_normal);
        if (!normal || !std::isfinite(g.inv_normal)) return RTW_E_INVALID;
        g.normal = normal;
        g.terms |= GUIDE_NORMAL;
    }
    if (p->same_object) {
        if (!idx) return RTW_E_INVALID;
        g.idx = idx;
        g.terms |= GUIDE_IDX;
    }
    return RTW_OK;
}

// host_filter_rows with the guide weight on every tap (TERMS == 0: the same arithmetic as host_filter_rows, nothing multiplied)
template <int TERMS>
void host_guided_rows(const uint8_t *img, uint32_t w, uint32_t h, uint32_t size, bool edges, const Plan &pl, const float *table,
                      const GuideArgs &ga, uint8_t *out, uint32_t y_begin, uint32_t y_end) {
    for (uint32_t y = y_begin; y < y_end; y++)
        for (uint32_t x = 0; x < w; x++) {
            const uint8_t *p = img + 3 * ((size_t)y * w + x);
            const GuidePixel gp = guide_load<TERMS>(ga.depth, ga.normal, ga.idx, (size_t)y * w + x);
            const uint32_t left = x - std::min(x, size), right = x + std::min(w - x - 1, size);
            const uint32_t up = y - std::min(y, size), down = y + std::min(h - y - 1, size);
            float col[3] = { 0, 0, 0 }, ws[3] = { 0, 0, 0 };
            for (uint32_t xi = left; xi < right; xi++)
                for (uint32_t yi = up; yi < down; yi++) {
                    const int dx = (int)xi - (int)x, dy = (int)yi - (int)y;
                    if (edges && !((uint32_t)(std::abs(dx) + std::abs(dy)) < size)) continue;
                    const float *t = table + 256u * pl.rowmap[dx * dx + dy * dy];
                    const uint8_t *q = img + 3 * ((size_t)yi * w + xi);
                    float g = 1.0f;
                    if (TERMS) g = guide_weight<TERMS>(ga.inv_depth, ga.inv_normal, gp, guide_load<TERMS>(ga.depth, ga.normal, ga.idx, (size_t)yi * w + xi));
                    for (int c = 0; c < 3; c++) {
                        float wt = t[std::abs((int)q[c] - (int)p[c])];
                        if (TERMS) wt = wt * g;
                        col[c] += ((float)q[c] * wt) / 255.0f;
                        ws[c] += wt;
                    }
                }
            for (int c = 0; c < 3; c++) out[3 * ((size_t)y * w + x) + c] = rust_as_u8((col[c] * 255.0f) / ws[c]);
        }
}

using HostGuidedRows = void (*)(const uint8_t *, uint32_t, uint32_t, uint32_t, bool, const Plan &, const float *, const GuideArgs &, uint8_t *,
                                uint32_t, uint32_t);
HostGuidedRows host_guided_rows_for(int terms) {
    static const HostGuidedRows f[8] = { host_guided_rows<0>, host_guided_rows<1>, host_guided_rows<2>, host_guided_rows<3>,
                                         host_guided_rows<4>, host_guided_rows<5>, host_guided_rows<6>, host_guided_rows<7> };
    return f[terms & 7];
}

double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

} // namespace

// ---- device path ---------------------------------------------------------------------------------------------------------------------
struct FilterScratch {
    DevMem img;                                    // the u8 frame on the device (copied or quantised)
    DevMem f32;                                    // a host f32 frame, staged for the quantise kernel
    DevMem terms;                                  // the gradient terms
    DevMem table;                                  // weight table [rows][256] f32, then the d2 -> row map
    DevMem out;                                    // the u8 result when the caller's buffer is host memory
    DevMem depth, normal, idx;                     // the guided filter's guides when the caller's are host memory
    DevMem sum;                                    // the gradient sum (device) ...
    PinnedMem h_sum;                               // ... and its pinned read-back slot
    PinnedMem h_table;                             // pinned: the table's upload is a true async copy
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
};

void filter_scratch_free(FilterScratch *f) {
    if (!f) return;
    for (hipEvent_t e : f->ev) if (e) (void)hipEventDestroy(e);
    delete f;                                      // (the buffers free themselves)
}

namespace {
float event_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f;
}
} // namespace

#define FILTER_TRY(expr)                                                                                                          \
    do {                                                                                                                          \
        hipError_t e_ = (expr);                                                                                                   \
        if (e_ != hipSuccess) { *last_hip = (int)e_; return e_ == hipErrorOutOfMemory ? RTW_E_NOMEM : RTW_E_HIP; } \
    } while (0)

namespace {
// What both filters do before their kernel: the scratch, the u8 frame on the device, the range term, the weight table and its upload.
struct Prepared {
    FilterScratch *f = nullptr;
    const uint8_t *img = nullptr;
    float avg = 0.0f, gradient_ms = 0.0f, table_ms = 0.0f;
    bool edges = false;
    Plan pl;
    size_t n_bytes = 0, n_rows = 0, table_bytes = 0;
};

int prepare_filter(int device, hipStream_t stream, FilterScratch **scratch, const void *in, uint32_t w, uint32_t h, const RtwBilateral *p,
                   Prepared &pr, int *last_hip) {
    FILTER_TRY(hipSetDevice(device));
    if (!*scratch) {
        FilterScratch *f = new (std::nothrow) FilterScratch();
        if (!f) return RTW_E_NOMEM;
        *scratch = f;
        for (hipEvent_t &e : f->ev) FILTER_TRY(hipEventCreate(&e));
        FILTER_TRY(f->sum.reserve(sizeof(float)));
        FILTER_TRY(f->h_sum.reserve(sizeof(float)));
    }
    FilterScratch *f = pr.f = *scratch;
    const size_t n_bytes = pr.n_bytes = (size_t)w * h * 3;

    // the u8 frame on the device
    const uint8_t *img;
    if (p->in_format == RTW_PIXELS_U8) {
        if (on_device(in, device)) img = (const uint8_t *)in;
        else {
            FILTER_TRY(f->img.reserve(n_bytes));
            FILTER_TRY(hipMemcpyAsync(f->img.ptr, in, n_bytes, hipMemcpyDefault, stream));
            img = f->img.as<uint8_t>();
        }
    } else {
        const float *src = (const float *)in;
        if (!on_device(in, device)) {
            FILTER_TRY(f->f32.reserve(n_bytes * sizeof(float)));
            FILTER_TRY(hipMemcpyAsync(f->f32.ptr, in, n_bytes * sizeof(float), hipMemcpyDefault, stream));
            src = f->f32.as<float>();
        }
        FILTER_TRY(f->img.reserve(n_bytes));
        hipLaunchKernelGGL(bilateral_quantize_kernel, dim3((unsigned)((n_bytes + 255) / 256)), dim3(256), 0, stream, src, n_bytes, f->img.as<uint8_t>());
        FILTER_TRY(hipGetLastError());
        img = f->img.as<uint8_t>();
    }
    pr.img = img;

    // the range term: the gradient terms in parallel, their sum in the reference's order by one wave, read back
    float avg = p->avg_gradient, gradient_ms = 0.0f;
    if (!(avg > 0.0f)) {
        const uint32_t n = (w - 2) * (h - 2);
        FILTER_TRY(f->terms.reserve((size_t)n * sizeof(float)));
        FILTER_TRY(hipEventRecord(f->ev[0], stream));
        hipLaunchKernelGGL(bilateral_gradient_terms_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, img, w, n, f->terms.as<float>());
        hipLaunchKernelGGL(bilateral_gradient_sum_kernel, dim3(1), dim3(64), 0, stream, f->terms.as<const float>(), n, f->sum.as<float>());
        FILTER_TRY(hipGetLastError());
        FILTER_TRY(hipEventRecord(f->ev[1], stream));
        FILTER_TRY(hipMemcpyAsync(f->h_sum.ptr, f->sum.ptr, sizeof(float), hipMemcpyDeviceToHost, stream));
        FILTER_TRY(hipStreamSynchronize(stream));
        avg = avg_from_sum(*f->h_sum.as<float>(), w, h);
        gradient_ms = event_ms(f->ev[0], f->ev[1]);
    }
    pr.avg = avg;
    pr.gradient_ms = gradient_ms;

    // the weight table (host libm expf) and the d2 -> row map, uploaded together
    const auto t1 = std::chrono::steady_clock::now();
    pr.edges = p->proximity == RTW_PROXIMITY_EDGES;
    Plan &pl = pr.pl;
    make_plan(w, h, p->size, pr.edges, pl);
    const size_t n_rows = pr.n_rows = std::max<size_t>(1, pl.row_d2.size());
    const size_t table_bytes = pr.table_bytes = n_rows * 256 * sizeof(float), map_bytes = pl.rowmap.size() * sizeof(uint16_t);
    FILTER_TRY(f->h_table.reserve(table_bytes + map_bytes));
    std::memset(f->h_table.ptr, 0, table_bytes);
    build_table(pl, range_term(avg), f->h_table.as<float>());
    std::memcpy(f->h_table.as<char>() + table_bytes, pl.rowmap.data(), map_bytes);
    FILTER_TRY(f->table.reserve(table_bytes + map_bytes));
    FILTER_TRY(hipMemcpyAsync(f->table.ptr, f->h_table.ptr, table_bytes + map_bytes, hipMemcpyHostToDevice, stream));
    pr.table_ms = (float)ms_since(t1);
    return RTW_OK;
}

void fill_stats(RtwFilterStats *stats, const Prepared &pr, std::chrono::steady_clock::time_point t0) {
    if (!stats) return;
    stats->avg_gradient = pr.avg;
    stats->spatial = pr.pl.spatial;
    stats->gradient_ms = pr.gradient_ms;
    stats->table_ms = pr.table_ms;
    stats->filter_ms = event_ms(pr.f->ev[2], pr.f->ev[3]);
    stats->total_ms = (float)ms_since(t0);
    stats->taps = pr.pl.taps;
}
} // namespace

int bilateral_filter_device(int device, hipStream_t stream, FilterScratch **scratch, const void *in, uint32_t w, uint32_t h,
                            const RtwBilateral *p, uint8_t *out, RtwFilterStats *stats, int *last_hip) {
    const auto t0 = std::chrono::steady_clock::now();
    int rc = check_args(in, w, h, p, out);
    if (rc != RTW_OK) return rc;
    Prepared pr;
    rc = prepare_filter(device, stream, scratch, in, w, h, p, pr, last_hip);
    if (rc != RTW_OK) return rc;
    FilterScratch *f = pr.f;
    const uint8_t *img = pr.img;
    const bool edges = pr.edges;
    const size_t n_bytes = pr.n_bytes, n_rows = pr.n_rows, table_bytes = pr.table_bytes;

    // the filter
    uint8_t *dst = out;
    const bool direct = on_device(out, device);
    if (!direct) { FILTER_TRY(f->out.reserve(n_bytes)); dst = f->out.as<uint8_t>(); }
    const int s = (int)p->size;
    const size_t tile_bytes = (size_t)(FBX + 2 * s) * (FBY + 2 * s) * sizeof(uint32_t);
    const bool table_lds = table_bytes + tile_bytes <= TABLE_LDS_MAX;
    const size_t lds = tile_bytes + (table_lds ? table_bytes : 0);
    const void *kern = table_lds ? (const void *)bilateral_filter_kernel<true> : (const void *)bilateral_filter_kernel<false>;
    if (lds > 64u * 1024u) FILTER_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid((w + FBX - 1) / FBX, (h + FBY - 1) / FBY);
    const float *d_table = f->table.as<float>();
    const uint16_t *d_map = (const uint16_t *)(f->table.as<char>() + table_bytes);
    FILTER_TRY(hipEventRecord(f->ev[2], stream));
    if (table_lds)
        hipLaunchKernelGGL(bilateral_filter_kernel<true>, grid, dim3(FBX * FBY), lds, stream, img, w, h, s, (int)edges, d_table,
                           (uint32_t)(n_rows * 256), d_map, dst);
    else
        hipLaunchKernelGGL(bilateral_filter_kernel<false>, grid, dim3(FBX * FBY), lds, stream, img, w, h, s, (int)edges, d_table,
                           (uint32_t)(n_rows * 256), d_map, dst);
    FILTER_TRY(hipGetLastError());
    FILTER_TRY(hipEventRecord(f->ev[3], stream));
    if (!direct) FILTER_TRY(hipMemcpyAsync(out, dst, n_bytes, hipMemcpyDefault, stream));
    FILTER_TRY(hipStreamSynchronize(stream));
    fill_stats(stats, pr, t0);
    return RTW_OK;
}

// ---- the guided filter on the device -------------------------------------------------------------------------------------------------
namespace {
using GuidedKernel = void (*)(const uint8_t *, uint32_t, uint32_t, int, int, const float *, uint32_t, const uint16_t *, const float *,
                              const float *, const int32_t *, float, float, uint8_t *);
template <int TERMS>
GuidedKernel guided_kernel_of(bool table_lds, bool guide_lds) {
    if (table_lds) return guide_lds ? guided_filter_kernel<true, true, TERMS> : guided_filter_kernel<true, false, TERMS>;
    return guide_lds ? guided_filter_kernel<false, true, TERMS> : guided_filter_kernel<false, false, TERMS>;
}
GuidedKernel guided_kernel_for(int terms, bool table_lds, bool guide_lds) {
    switch (terms & 7) {
    case 0: return guided_kernel_of<0>(table_lds, false);          // no guide: nothing to place
    case 1: return guided_kernel_of<1>(table_lds, guide_lds);
    case 2: return guided_kernel_of<2>(table_lds, guide_lds);
    case 3: return guided_kernel_of<3>(table_lds, guide_lds);
    case 4: return guided_kernel_of<4>(table_lds, guide_lds);
    case 5: return guided_kernel_of<5>(table_lds, guide_lds);
    case 6: return guided_kernel_of<6>(table_lds, guide_lds);
    default: return guided_kernel_of<7>(table_lds, guide_lds);
    }
}

// Where the weight table and the guide tile go (profiles/guided_lds_ab.log).  layout 0 decides by size; 1 .. 4 ask for
// table + guides in LDS / guides only / table only / neither, and are followed where the request fits in GUIDED_LDS_CAP.
void guided_layout(uint32_t layout, size_t table_bytes, size_t tile_bytes, size_t guide_bytes, bool &table_lds, bool &guide_lds) {
    guide_lds = guide_bytes > 0 && tile_bytes + guide_bytes <= GUIDED_GUIDE_LDS_MAX;
    table_lds = table_bytes + tile_bytes + (guide_lds ? guide_bytes : 0) <= GUIDED_TABLE_LDS_MAX;
    if (layout >= 1 && layout <= 4) {
        const bool t = layout == 1 || layout == 3, g = guide_bytes > 0 && (layout == 1 || layout == 2);
        if (tile_bytes + (t ? table_bytes : 0) + (g ? guide_bytes : 0) <= GUIDED_LDS_CAP) { table_lds = t; guide_lds = g; }
    }
}
} // namespace

int guided_filter_device(int device, hipStream_t stream, FilterScratch **scratch, uint32_t layout, const void *in, uint32_t w, uint32_t h,
                         const float *depth, const float *normal, const int32_t *idx, const RtwGuidedFilter *p, uint8_t *out,
                         RtwFilterStats *stats, int *last_hip) {
    const auto t0 = std::chrono::steady_clock::now();
    GuideArgs ga;
    int rc = check_guided_args(in, w, h, depth, normal, idx, p, out, ga);
    if (rc != RTW_OK) return rc;
    Prepared pr;
    rc = prepare_filter(device, stream, scratch, in, w, h, &p->base, pr, last_hip);
    if (rc != RTW_OK) return rc;
    FilterScratch *f = pr.f;

    // the guides on the device: a host plane is staged; a plane whose term is off is not touched
    const size_t n_px = (size_t)w * h;
    if (ga.depth && !on_device(ga.depth, device)) {
        FILTER_TRY(f->depth.reserve(n_px * sizeof(float)));
        FILTER_TRY(hipMemcpyAsync(f->depth.ptr, ga.depth, n_px * sizeof(float), hipMemcpyDefault, stream));
        ga.depth = f->depth.as<const float>();
    }
    if (ga.normal && !on_device(ga.normal, device)) {
        FILTER_TRY(f->normal.reserve(n_px * 3 * sizeof(float)));
        FILTER_TRY(hipMemcpyAsync(f->normal.ptr, ga.normal, n_px * 3 * sizeof(float), hipMemcpyDefault, stream));
        ga.normal = f->normal.as<const float>();
    }
    if (ga.idx && !on_device(ga.idx, device)) {
        FILTER_TRY(f->idx.reserve(n_px * sizeof(int32_t)));
        FILTER_TRY(hipMemcpyAsync(f->idx.ptr, ga.idx, n_px * sizeof(int32_t), hipMemcpyDefault, stream));
        ga.idx = f->idx.as<const int32_t>();
    }

    uint8_t *dst = out;
    const bool direct = on_device(out, device);
    if (!direct) { FILTER_TRY(f->out.reserve(pr.n_bytes)); dst = f->out.as<uint8_t>(); }
    const int s = (int)p->base.size;
    const size_t tile_bytes = (size_t)(FBX + 2 * s) * (FBY + 2 * s) * sizeof(uint32_t);
    const size_t guide_bytes = tile_bytes * guide_planes(ga.terms);
    bool table_lds, guide_lds;
    guided_layout(layout, pr.table_bytes, tile_bytes, guide_bytes, table_lds, guide_lds);
    const size_t lds = tile_bytes + (table_lds ? pr.table_bytes : 0) + (guide_lds ? guide_bytes : 0);
    const GuidedKernel kern = guided_kernel_for(ga.terms, table_lds, guide_lds);
    if (lds > 64u * 1024u) FILTER_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid((w + FBX - 1) / FBX, (h + FBY - 1) / FBY);
    const float *d_table = f->table.as<float>();
    const uint16_t *d_map = (const uint16_t *)(f->table.as<char>() + pr.table_bytes);
    FILTER_TRY(hipEventRecord(f->ev[2], stream));
    hipLaunchKernelGGL(kern, grid, dim3(FBX * FBY), lds, stream, pr.img, w, h, s, (int)pr.edges, d_table, (uint32_t)(pr.n_rows * 256), d_map,
                       ga.depth, ga.normal, ga.idx, ga.inv_depth, ga.inv_normal, dst);
    FILTER_TRY(hipGetLastError());
    FILTER_TRY(hipEventRecord(f->ev[3], stream));
    if (!direct) FILTER_TRY(hipMemcpyAsync(out, dst, pr.n_bytes, hipMemcpyDefault, stream));
    FILTER_TRY(hipStreamSynchronize(stream));
    fill_stats(stats, pr, t0);
    return RTW_OK;
}
#undef FILTER_TRY

} // namespace rtw

// ---- host path -----------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(RtwBilateral) == 16 && sizeof(RtwFilterStats) == 32, "POD layout");
static_assert(offsetof(RtwFilterStats, taps) == 24, "RtwFilterStats has no padding");

static_assert(sizeof(RtwGuidedFilter) == 28 && offsetof(RtwGuidedFilter, sigma_depth) == 16, "POD layout");

namespace rtw {
namespace {
// both host filters after their argument checks; ga == nullptr: the plain one
int host_filter(const void *in, uint32_t w, uint32_t h, const RtwBilateral *p, const GuideArgs *ga, uint8_t *out, RtwFilterStats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n_bytes = (size_t)w * h * 3;
    std::vector<uint8_t> quantised;
    const uint8_t *img = (const uint8_t *)in;
    if (p->in_format == RTW_PIXELS_F32_RUST2) {
        quantised.resize(n_bytes);
        rtw_quantize_u8_rust2((const float *)in, n_bytes, quantised.data());
        img = quantised.data();
    }
    float avg = p->avg_gradient, gradient_ms = 0.0f;
    if (!(avg > 0.0f)) {
        const auto tg = std::chrono::steady_clock::now();
        avg = avg_from_sum(host_gradient_sum(img, w, h), w, h);
        gradient_ms = (float)ms_since(tg);
    }
    const auto t1 = std::chrono::steady_clock::now();
    const bool edges = p->proximity == RTW_PROXIMITY_EDGES;
    Plan pl;
    make_plan(w, h, p->size, edges, pl);
    std::vector<float> table(std::max<size_t>(1, pl.row_d2.size()) * 256, 0.0f);
    build_table(pl, range_term(avg), table.data());
    const float table_ms = (float)ms_since(t1);
    const auto t2 = std::chrono::steady_clock::now();
    // pixels are independent: rows are split over up to 16 threads (the result does not depend on the split)
    const uint32_t n_threads = std::max(1u, std::min({ std::thread::hardware_concurrency(), 16u, h }));
    const uint32_t per = (h + n_threads - 1) / n_threads;
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n_threads; t++) {
        const uint32_t a = std::min(h, t * per), b = std::min(h, a + per);
        if (a >= b) continue;
        if (ga) pool.emplace_back(host_guided_rows_for(ga->terms), img, w, h, p->size, edges, std::cref(pl), table.data(), std::cref(*ga), out, a, b);
        else pool.emplace_back(host_filter_rows, img, w, h, p->size, edges, std::cref(pl), table.data(), out, a, b);
    }
    if (ga) host_guided_rows_for(ga->terms)(img, w, h, p->size, edges, pl, table.data(), *ga, out, 0, std::min(h, per));
    else host_filter_rows(img, w, h, p->size, edges, pl, table.data(), out, 0, std::min(h, per));
    for (std::thread &t : pool) t.join();
    if (stats) {
        stats->avg_gradient = avg;
        stats->spatial = pl.spatial;
        stats->gradient_ms = gradient_ms;
        stats->table_ms = table_ms;
        stats->filter_ms = (float)ms_since(t2);
        stats->total_ms = (float)ms_since(t0);
        stats->taps = pl.taps;
    }
    return RTW_OK;
}
} // namespace
} // namespace rtw

extern "C" int rtw_bilateral_filter(const void *in, uint32_t w, uint32_t h, const RtwBilateral *p, uint8_t *out, RtwFilterStats *stats) {
    const int rc = rtw::check_args(in, w, h, p, out);
    return rc != RTW_OK ? rc : rtw::host_filter(in, w, h, p, nullptr, out, stats);
}

extern "C" int rtw_guided_filter(const void *in, uint32_t w, uint32_t h, const float *depth, const float *normal, const int32_t *idx,
                                 const RtwGuidedFilter *p, uint8_t *out, RtwFilterStats *stats) {
    rtw::GuideArgs ga;
    const int rc = rtw::check_guided_args(in, w, h, depth, normal, idx, p, out, ga);
    return rc != RTW_OK ? rc : rtw::host_filter(in, w, h, &p->base, &ga, out, stats);
}
