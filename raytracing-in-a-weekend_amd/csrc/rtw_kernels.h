// rtw_kernels.h -- kernel argument block shared by rtw_kernels.hip (device) and rtw_shim.hip (host).
#pragma once
#include "rtw_device.h"
#include "rtw_tri.h"
#include "rtw_light.h"
#include "rtw_mixed.h"
#include "rtw_host.h"
#include <type_traits>

#define RTW_QUEUE_BYTES 4096u   // the work queue's counters (KArgs.queue): up to 8 sub-queues ...
#define RTW_QUEUE_STRIDE 256u   // ... bytes apart
#ifndef RTW_SUB_SHIFT
#define RTW_SUB_SHIFT 3u        // log2 of the number of sub-queues (8: one per XCD; 16 and 32 measured no better, profiles/r02_subq_count.log)
#endif
#define RTW_N_STATS 64  // 64-bit counters a render launch accumulates (KArgs.stats); [32..63] are used by the -DRTW_CENSUS diagnostic build only
#ifndef RTW_LIST_WALK_MAX_DEFAULT
#define RTW_LIST_WALK_MAX_DEFAULT 48u  // RTW_OPT_LIST_WALK_MAX: scenes this small walk the list even when the BVH is asked for (measured crossover ~56 spheres: profiles/r02_crossover.log)
#endif
#ifndef RTW_MESH_LIST_MAX_DEFAULT
#define RTW_MESH_LIST_MAX_DEFAULT 16u  // RTW_OPT_MESH_LIST_MAX: this few placements are met in list order even when the BVH is asked for (measured: the largest count at which the list is not slower, profiles/mesh_top_tree.log)
#endif

namespace rtw {

// Device view of the acceleration structure built by build_bvh() (rtw_host.cpp).
struct DevBvh {
    const BvhNode *nodes;
    const BvhNode16 *nodes16;     // f16 copy for the LDS-resident variant, or null
    uint32_t n_nodes;
    const f4 *big_geom;           // {cx, cy, cz, r*r} of the spheres kept outside the tree
    const f4 *big_vel;
    const uint32_t *big_index;    // their indices in the scene list
    uint32_t n_big;
    uint32_t depth;               // tree depth (the stack needs depth + 3 levels: sentinel, one per level, the slot above the top)
    int32_t root;                 // node index; ~sphere when the tree is a single leaf; INT32_MIN when empty
    float cx, cy, cz;             // centre C of the tree spheres' centres
    float centre_radius;          // R_c
    float r_max2;                 // r_max^2
    float inv_2rmin;              // 1 / (2 r_min), +inf when r_min == 0
    float abs_max;                // largest |coordinate| of the root box
};

struct KArgs {
    RtwCamera cam;
    DevScene  sc;
    DevBvh    bvh;
    DevGeom   geom;               // quads and instances (n_quads == n_inst == 0 for sphere-only scenes)
    uint32_t width, height;       // full image
    uint32_t k_base, k_end;       // compact rows [k_base, k_end) of this partition rendered by this launch (a band)
    uint32_t n_tiles;             // tiles_x * ceil((k_end - k_base) / 8)
    uint32_t chunk_len, n_chunks; // samples per work unit and units per pixel of the queue's FIRST region (all of it with RTW_FLAG_CHUNK_SUMS)
    uint32_t bank_len;            // 0: the bank holds one slot per sample, [tile][sample][pixel] -- independent of how the samples are cut into units;
                                  // 1 (RTW_FLAG_CHUNK_SUMS): one slot per unit, [tile][chunk][pixel]
    // The unit length is GUIDED within a launch: the tiles at queue positions [0, reg_q1) are cut into units of reg_len[0] samples, [reg_q1, reg_q2) into
    // units of reg_len[1], the rest -- the end of the queue -- into units of reg_len[2] (reg_nc[r] = ceil(n_samples / reg_len[r]) units per pixel):
    // long units amortise the per-unit work while plenty is left, short ones keep the drain of the launch short (rtw_shim.hip)
    uint32_t reg_q1, reg_q2;
    uint32_t reg_len[3], reg_nc[3];
    uint32_t flags;               // RtwParams.flags (RTW_FLAG_CPP_*: generic build only)
    float *samples;               // per-sample radiance, [n_tiles][n_samples][64][3]  (RTW_FLAG_CHUNK_SUMS: [n_tiles][n_chunks][64][3])
    uint32_t row_block, part_index, part_count;
    uint32_t tiles_x;             // ceil(width / 8)
    uint32_t total_work;          // work items of the launch: 64 per (tile, unit)
    uint32_t sub_shift;           // the work queue is 2^sub_shift sub-queues (tiles dealt round-robin in queue order), counters RTW_QUEUE_STRIDE bytes apart
    uint32_t grab_shift, grab_max;   // a wave takes min(grab_max, (work left >> grab_shift) rounded down to whole blocks, at least one block) items per queue atomic
    const uint32_t *tile_order;   // queue position -> tile (a permutation of [0, n_tiles)), or null = raster order
    uint32_t n_samples;           // rays per pixel actually traced (sampler-dependent)
    uint32_t s_root;              // strata per axis (STRATIFIED / CENTRES)
    uint32_t sampler, integrator, depth;
    uint32_t has_textures;        // any sphere with an image texture (a fact render_need reads: the common configuration's build that keeps the lookup)
    uint32_t lds_bytes;           // dynamic LDS of the BVH kernel: nodes | stack | sphere geometry (rtw_host.h render_lds_layout, which sets all three)
    uint32_t lds_stack_off, lds_geom_off;   // byte offsets (16-aligned) of the per-lane stack and of the sphere geometry, which the NODES == 2
                                            // builds alone read; the nodes sit at offset 0
    uint32_t seed_lo, seed_hi;
    float inv_gamma, mint, maxt;
    float bg[3];
    float *out;                   // [rows of the partition][width][3]
    uint32_t *queue;              // work-item counter, zeroed before launch
    unsigned long long endtimes_ref;   // -DRTW_ENDTIMES builds: reference wave lifetime for the histogram (0 = none)
    unsigned long long *stats;    // [0] camera rays [1] segments [2] sphere tests [3] node tests [4] nan pixels [5..7] phase steps [8..10] phase lanes [14] quad tests [16..19] steps, lanes of phases 3 (switch), 4 (new path)
    // (appended: the offsets of everything above, which the other builds read, stay where they were)
    DevNoise noise;               // texture noise (rtw_ctx_set_texture_noise); noise.tex != null selects the noise build (SPEC 7), which alone reads it
    DevTris tris;                 // Rust2 triangles (rtw_ctx_set_triangles); tris.n != 0 selects the triangle build (SPEC 8), which alone reads it;
                                  // tris.nodes == null: walk the triangle list
    DevLights lights;             // the light list (rtw_ctx_set_lights); read by the light build (SPEC 9) alone, which RTW_INTEGRATOR_LIGHT_CAST /
                                  // _LIGHT_BIASED select
    const f4 *inst_quats;         // Rust2's instance rotations (rtw_ctx_set_instance_rotations): one normalised {w, x, y, z} per instance; non-null selects
                                  // the quaternion build (SPEC 11), which alone reads it (and the lights, for every integrator it serves)
    const f4 *mesh_rows;          // mesh placements (rtw_ctx_set_mesh_instances): two rows {qn}, {position, 0} per placement (rtw_mesh.h); non-null selects
    uint32_t n_mesh;              // the placement build (SPEC 12), which alone reads them: tris is then the mesh every placement shares
    const uint32_t *nodes32;      // the tree's f32 plane format (rtw_host.h pack_nodes32): what the large-workgroup builds copy into LDS instead of
                                  // bvh.nodes16; they alone read it, and it is set for them alone (LdsLayout.node_format == 2)
    const TriNode *mesh_top;      // the top-level tree over the placements (rtw_mesh.h mesh_top_walk; the order array sits behind the nodes), or
    uint32_t n_mesh_top;          // null: the placements are met in list order.  Read by the placement build alone
};

// One instantiation of render_brute<MOVING, SPEC, GEOM> / render_bvh<MOVING, NODES, SPEC, GEOM> (nodes: 0 for render_brute): what a launch
// runs and what rtw_ctx_last_render_build reports are this one value.
struct RenderBuild { bool bvh, moving, geom; int nodes, spec; };
typedef void (*render_fn)(const KArgs);
// The kernel of a build, or null: none is compiled for these five values
render_fn render_kernel(const RenderBuild &b);
// Its threads per workgroup: RTW_BLOCK, or RTW_BLOCK_LARGE for the builds that walk the f32 plane format (bvh_block of the same five values)
uint32_t render_block(const RenderBuild &b);
// The render kernel with a.lds_bytes of dynamic LDS, then the in-order resolve of the band, on `stream`
void launch_render(render_fn fn, uint32_t block, const KArgs &a, uint32_t grid, hipStream_t stream);
// rtw_ctx_perlin_eval: out[i] = perlin_eval(*t, points[i], depth) for i < n (device pointers), on `stream`
void launch_perlin_eval(const RtwPerlin *t, const float *points, uint32_t n, uint32_t depth, float *out, hipStream_t stream);
// rtw_ctx_triangle_hits: the closest triangle of T for each of n rays ([n][6] = o, d; device pointers), on `stream`; counters[0] triangle
// tests, [1] node visits (device u64, accumulated)
void launch_tri_hits(const DevTris &T, const float *rays, uint32_t n, float mint, float maxt, float *t_out, int32_t *idx_out,
                     unsigned long long *counters, hipStream_t stream);
// N runtime bools as N compile-time ones: f(std::bool_constant<b0>{}, ..., std::bool_constant<bN-1>{}), all 2^N calls of one return type.
// How every launch_* below gets from its arguments to the kernel instantiation.
template <bool... Done, class F>
auto with_bools(F f) { return f(std::bool_constant<Done>{}...); }
template <bool... Done, class F, class... Rest>
auto with_bools(F f, bool b, Rest... rest) { return b ? with_bools<Done..., true>(f, rest...) : with_bools<Done..., false>(f, rest...); }
// rtw_ctx_scene_hits / rtw_ctx_depth_map (rtw_query.hip): one closest-hit query per ray over spheres, quads, instances and triangles.
struct QueryArgs {
    DevScene sc;
    DevBvh   bvh;
    DevGeom  geom;
    DevTris  tris;                // tris.n == 0: none; tris.nodes == null: walk the triangle list
    const f4 *inst_quats;         // Rust2's instance rotations, one normalised {w, x, y, z} per instance, or null: the Euler rotation of DevInstance
    const f4 *mesh_rows;          // mesh placements, two rows per placement (rtw_mesh.h), or null: tris is a world-space group
    uint32_t n_mesh;
    const TriNode *mesh_top;      // the top-level tree over the placements, or null (as in KArgs)
    uint32_t n_mesh_top;
    RtwCamera cam;                // from_camera: Rust2's camera (rtw_camera2_new), pixel i = (i % width, i / width)
    uint32_t width, height;
    const float *rays;            // else: [n][6] = o, d (device)
    uint32_t n;
    uint32_t levels;              // tree: levels of the per-lane LDS stack (DevBvh.depth + 2: the sentinel, one per tree level)
    float time, mint, maxt;
    float miss_t;                 // t_out of a miss: +inf (scene_hits) or maxt * 1.6 (depth_map, Rust2/src/viewport.rs:68)
    float span;                   // tree: the farthest a sphere centre reaches (rtw_ctx.scene_span), for the per-ray check
    float *t_out;                 // [n]
    int32_t *idx_out;             // [n] or null
    float *normal_out;            // [n][3] or null
    unsigned long long *counters; // RTW_QUERY_SLOTS lines of RTW_QUERY_STRIDE counters, a workgroup adds to line blockIdx % RTW_QUERY_SLOTS (the host sums
                                  // the lines): [0] sphere tests [1] node visits (both trees) [2] quad + triangle tests [3] waves whose stack was too short
    // rtw_ctx_scene_surface / rtw_ctx_surface_map: read by the SURF builds of scene_hits_kernel only, which albedo_out != null selects
    float *albedo_out;            // [n][3]
    float *emitted_out;           // [n][3] or null
    float *material_out;          // [n][3] = metallicness, opacity, ir; or null
    uint32_t rust2;               // the record follows Rust2's texel rules (RTW_INTEGRATOR_RUST2, _LIGHT_CAST, _LIGHT_BIASED)
    uint32_t ray_rule;            // from_camera: RTW_RAYS_DEPTH_MAP | RTW_RAYS_PIXEL
    float off_x, off_y;           // RTW_RAYS_PIXEL: the offset inside the pixel
    // rtw_ctx_scene_surface_tri / rtw_ctx_surface_map_tri: the SURF builds only; at the END, so that no offset above moves
    int32_t *tri_out;             // [n] or null: the winning triangle's position in the caller's list (win 3 or 4), else -1
    float *bary_out;              // [n][2] or null: its (alfa, beta) as tri_inside forms them on the ray tri_record is given, else 0 0
};
#define RTW_QUERY_SLOTS 64u       // one atomic per wave and counter, spread over 64 cache lines: tens of thousands of waves adding to ONE line serialise
#define RTW_QUERY_STRIDE 16u      // counters (u64) per line: 128 bytes
// from_camera: rays built from q.cam, else read from q.rays; tree: the sphere group through DevBvh.nodes (dynamic LDS = levels * RTW_BLOCK * 4)
void launch_scene_hits(const QueryArgs &q, bool from_camera, bool tree, hipStream_t stream);
// rtw_ctx_scene_occluded (rtw_occluded.hip): one any-hit query per ray over the same four groups; the fields are QueryArgs' of the same names.
struct OccludedArgs {
    DevScene sc;
    DevBvh   bvh;
    DevGeom  geom;
    DevTris  tris;
    const f4 *inst_quats;
    const f4 *mesh_rows;
    uint32_t n_mesh;
    const TriNode *mesh_top;
    uint32_t n_mesh_top;
    const float *rays;            // [n][6] = o, d (device)
    uint32_t n;
    uint32_t levels;
    float time, mint, maxt;
    float span;
    uint8_t *out;                 // [n]: 1 = something accepts the ray within [mint, maxt], else 0
    unsigned long long *counters; // as QueryArgs.counters
};
// tree: the sphere group through DevBvh.nodes (dynamic LDS = levels * RTW_BLOCK * 4)
void launch_scene_occluded(const OccludedArgs &q, bool tree, hipStream_t stream);
// rtw_ctx_ambient_occlusion / rtw_ctx_ao_map (rtw_occluded.hip): `samples` any-hit rays per point, made in the kernel by
// the rule of rtw_ao.h, one float per point.  q: the scene views, [mint, maxt] of the AO rays, the counters ([4]: the points that cast
// rays); q.n is the number of POINTS, q.rays and q.out are not read.
struct AoArgs {
    OccludedArgs q;
    const float *points;          // [n][3] (device); from_camera: not read
    const float *normals;         // [n][3] (device); from_camera: the depth pass's normals of the pixels
    uint32_t samples, seed;       // samples: a power of two in 1 .. 1024
    uint32_t lg_group;            // log2 of the lanes that share a point: min(samples, 64)
    float *ao_out;                // [n]
    RtwCamera cam;                // from_camera: as QueryArgs.cam, point j * width + i is pixel (i, j) ...
    uint32_t width, height;
    const float *depth;           // ... at p = o + d * depth[pixel] with the normal faced towards the viewer,
    const int32_t *idx;           // skipped where idx[pixel] < 0 (device, what launch_scene_hits wrote)
};
// from_camera: the points come from the depth pass's outputs; tree: as launch_scene_occluded.  (samples <= 64 runs the single-round build)
void launch_ambient_occlusion(const AoArgs &q, bool from_camera, bool tree, hipStream_t stream);
// rtw_ctx_direct_light / rtw_ctx_direct_light_map (rtw_occluded.hip): `samples` any-hit segments per (point, light) pair,
// made in the kernel by the rule of rtw_direct.h, two floats per pair.  q: the scene views, [lo, hi] of the segments, the counters ([4]: the
// rays cast); q.n is the number of POINTS, q.rays and q.out are not read.  The other fields are AoArgs' of the same names.
struct DirectRow;
struct DirectArgs {
    OccludedArgs q;
    const float *points;          // [n][3] (device); from_camera: not read
    const float *normals;         // [n][3] (device); from_camera: the depth pass's normals of the pixels
    const DirectRow *lights;      // [n_lights] rows (device; rtw_direct.h)
    uint32_t n_lights;            // 1 .. RTW_MAX_LIGHTS; item i * n_lights + l is point i under light l
    uint32_t samples, seed;       // samples: a power of two in 1 .. 1024
    uint32_t lg_group;            // log2 of the lanes that share an item: min(samples, 64)
    float *vis_out;               // [n][n_lights]
    float *irr_out;               // [n][n_lights] or null
    RtwCamera cam;
    uint32_t width, height;
    const float *depth;
    const int32_t *idx;
};
void launch_direct_light(const DirectArgs &q, bool from_camera, bool tree, hipStream_t stream);
// rtw_ctx_mesh_instance_hits: the closest placement of mesh T for each of n rays through mesh_closest (rtw_mesh.h); placement / triangle
// -1 and t +inf on a miss; normal_out ([n][3]) may be null; counters as launch_tri_hits
void launch_mesh_hits(const DevTris &T, const f4 *rows, uint32_t n_mesh, const TriNode *top, uint32_t n_top, const float *rays, uint32_t n, float mint, float maxt, float *t_out,
                      int32_t *placement_out, int32_t *tri_out, float *normal_out, unsigned long long *counters, hipStream_t stream);

} // namespace rtw
