// rtw_host.h -- host-side C++ mirror of the reference constructors (Viewport::new, Sphere::new,
// Scene::new_sphere's acceleration build) and the BASELINE scene generators.  Pure host code.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "rtw.h"

namespace rtw {

// f32 helpers: this library is built with -ffp-contract=off, so these are single IEEE operations.
static inline float host_mul(float a, float b) { return a * b; }
static inline float host_div(float a, float b) { return a / b; }

// Rays per pixel a sampler traces for Viewport.samples (viewport.rs:443; Rust2 viewport.rs:90).
uint32_t sampler_count(uint32_t sampler, uint32_t samples, uint32_t *s_root);

// ---- acceleration structure ---------------------------------------------------------------------
// Binary BVH, single-sphere leaves, both child boxes stored in the parent (one 64-byte fetch per
// visit = two slab tests).  child >= 0: inner node index; child < 0: leaf holding sphere ~child.
struct BvhNode {
    float lo0[3], hi0[3];
    float lo1[3], hi1[3];
    int32_t c0, c1;
    uint32_t pad[2];
};
static_assert(sizeof(BvhNode) == 64, "BvhNode must be 64 bytes");

// Compact node for the LDS-resident variant: the same two child boxes as f16, rounded OUTWARD (lo down,
// hi up: the tree only prunes, so larger boxes stay conservative), 16-bit child ids.  32 bytes.
// One dword per (box, axis) holding {lo, hi}: the kernel swaps the halves with ONE v_perm_b32 when the ray
// runs against the axis and has its {near plane, far plane} without a min / max pair.
struct BvhNode16 {
    uint16_t plane[2][3][2];   // [child box][axis]{lo, hi}
    int16_t c0, c1;
    uint32_t pad;
};
static_assert(sizeof(BvhNode16) == 32, "BvhNode16 must be 32 bytes");
#define RTW_LDS_NODES_MAX 512 // inner nodes the LDS variant holds (16 KB)
#define RTW_LDS_GEOM_MAX 640  // spheres whose {centre, r^2} the LDS variant also keeps on chip for the leaf tests (10 KB)

// The same node with its planes widened to f32 (exactly: every f16 value is an f32 value), for the render builds that read a ray's
// {near, far} pair straight out of LDS at a per-ray address instead of permuting and widening it (rtw_kernels.hip trav_node_lds32).
// RTW_NODE32_DWORDS (28) dwords per node: per (box, axis), in BvhNode16's order, a group of four planes {hi, lo, lo, hi} -- a pair read
// RTW_NODE32_OFF (8) bytes into the group is {lo, hi} (a ray along +axis), one read at its start {hi, lo} (along -axis); either read is
// 8-byte aligned (pairs at 4-byte alignment, out of {hi, lo, hi}, were measured ruinous: profiles/f32_planes_ab.log) -- then the dword
// {c0, c1} of 16-bit child codes at dwords 24 and 26, where a read at either per-ray offset finds it, so that it needs no address of its own,
// each followed (dwords 25 and 27) by the same two codes swapped, {c1, c0}: one 8-byte read hands the visit the pair in both orders.
// A leaf's code is BvhNode16's (~sphere); an inner child is named by its LDS offset in units of 8 bytes (1 << RTW_NODE32_UNIT_SHIFT):
// index * RTW_NODE32_CODE.  In bytes, as the f16 format names them, the last of Book-1's 480 nodes (53648) would not fit below the END /
// DEAD codes 0x7FFF / 0x7FFE of the 16-bit stack entries; in these units every tree with f16 nodes does (511 * 14 = 7154).
#define RTW_NODE32_AXIS_DWORDS 4u
#define RTW_NODE32_OFF 8u
#define RTW_NODE32_DWORDS 28u
#define RTW_NODE32_UNIT_SHIFT 3u
#define RTW_NODE32_CODE (RTW_NODE32_DWORDS * 4u >> RTW_NODE32_UNIT_SHIFT)   // 14
#define RTW_NODE32_NODES_MAX (0x7FFDu / RTW_NODE32_CODE + 1u)             // the code range's limit (2341 nodes); RTW_LDS_NODES_MAX binds first
static_assert(RTW_LDS_NODES_MAX <= RTW_NODE32_NODES_MAX, "every tree with f16 nodes has f32 planes");

#define RTW_MAX_BIG 16        // spheres far larger than the rest are tested exactly, outside the tree
#define RTW_BVH_STACK 24      // builder guarantees depth <= RTW_BVH_STACK (median-split fallback near the limit)
#define RTW_BVH_OPTIMISE_MAX 1024u    // tree spheres up to which the builder sweeps every split (n log n per level) and runs the reinsertion pass.
                                       // Larger scenes get the binned top-down tree alone.
#ifndef RTW_BVH_REINSERT_WORK
#define RTW_BVH_REINSERT_WORK 128u     // the reinsertion pass's work budget: search steps per tree node (set_scene is on the caller's path)
#endif

struct BvhBuild {
    std::vector<BvhNode> nodes;          // nodes[0] is the root (absent when < 2 tree spheres)
    std::vector<BvhNode16> nodes16;      // f16 copy, filled only when it is usable (see build_bvh)
    std::vector<uint32_t> big;           // sphere indices tested by the uniform pre-pass
    int32_t root;                        // node index, or ~sphere for a single tree sphere, or INT32_MIN if empty
    // per-ray padding constants (DESIGN.md "Conservative traversal"): over the TREE spheres only
    float centre[3];                     // C: centre of the box of sphere centres
    float centre_radius;                 // R_c: max |c_s - C| (time-expanded)
    float r_min, r_max;                  // radius range of the tree spheres
    float abs_max;                       // largest |coordinate| of any tree box
    uint32_t depth;
    uint32_t depth_cap;                  // the deepest level the builder allowed itself for this scene (bvh_depth_cap, or the caller's)
};

// How build_bvh builds.  The defaults are the product's; the others exist so that `scripts/sim/wave_sim visits` can price the alternatives.
struct BvhBuildOptions {
    bool sweep = true;                   // full-sweep SAH over all three axes (false: the 16-bin centroid SAH of the earlier builder)
    bool reinsert = true;                // subtree-reinsertion pass over the finished tree
    uint32_t depth_cap = 0;              // 0: bvh_depth_cap()
};
// The deepest level a leaf may sit on: for a tree that may live in LDS, the deepest at which the f16 nodes plus the per-lane stack
// still fit a seventh of a CU's LDS (the render kernel's seven workgroups per CU) and, where the shim would also keep the scene's
// n_spheres x 16 bytes of sphere geometry in LDS for a balanced tree (its sixth-of-a-CU rule), the deepest at which it still does;
// RTW_BVH_STACK otherwise; never less than a balanced tree needs.
uint32_t bvh_depth_cap(uint32_t n_leaves, uint32_t n_spheres, bool lds_candidate);

// Bounds cover centre(t) = origin + velocity * t for t in [t_begin, t_end] (sphere.rs:100); the
// reference's own AABB ignores velocity (aabb/aabb.rs:27-39) and so culls moving spheres wrongly.
void build_bvh(const RtwSphere *spheres, uint32_t n, float t_begin, float t_end, BvhBuild &out, const BvhBuildOptions &opt = BvhBuildOptions());

// The f32 plane format of a tree's f16 nodes (above): derived from nodes16 by widening, never a second rounding of the f32 boxes -- the
// walk over it is then the walk over nodes16, decision for decision.  Empty in, empty out.
void pack_nodes32(const std::vector<BvhNode16> &nodes16, std::vector<uint32_t> &out);

// ---- which render build a launch runs, and its dynamic LDS --------------------------------------------------------------------
// Three steps, each a function of plain values: render_need -- what the request needs --, render_lds_layout -- what the
// tree allows --, and the kernel of the RenderBuild the two name (rtw_kernels.h render_kernel).  rtw_shim.hip calls each once per render;
// rtw_render_choice (rtw.h) runs the same three without a device.
#ifndef RTW_BLOCK
#define RTW_BLOCK 256         // 4 waves per workgroup
#endif
#define RTW_BLOCK_LARGE 768   // 12 waves: the static LDS-node builds that walk f32 planes (rtw_kernels.hip bvh_block); two per CU
// A CU's LDS, and the shares of it the 256-thread builds are laid out for: a tree's f16 nodes and stack within a seventh (seven workgroups
// per CU, 7 waves per SIMD), the same with the spheres' geometry behind them within a sixth (six, the kernel's register budget).
#define RTW_CU_LDS_BYTES (160u * 1024u)
#define RTW_LDS_SHARE_TREE 7u
#define RTW_LDS_SHARE_GEOM 6u
static inline uint32_t lds_align16(uint32_t bytes) { return (bytes + 15u) & ~15u; }
// The per-lane traversal stack, [level][thread]: `levels` rows of `block` entries
static inline uint32_t lds_stack_bytes(uint32_t levels, uint32_t block, uint32_t entry_bytes) { return lds_align16(levels * block * entry_bytes); }

// The SPEC a request runs and whether it needs the GEOM stage (quads, instances, triangles, rotations, placements).  !geom is also
// "there is a build that reads the spheres' {centre, r^2} from LDS" (NODES == 2 exists without GEOM only).
struct RenderNeed { int spec; bool geom; };
RenderNeed render_need(const RtwRenderFacts &f);

// NODES and the dynamic LDS of a launch.  nodes / node_format / block: the NODES template argument, the LDS node format (0 none, 1 f16
// nodes, 2 f32 planes) and the threads per workgroup; stack_off / geom_off / tri_off / bytes: KArgs.lds_stack_off / lds_geom_off /
// tris.lds_off / lds_bytes (geom_off 0: the geometry stays in global memory; tri_off: the last 16 bytes of a request with triangles).
struct LdsLayout { int nodes; uint32_t node_format, block, stack_off, geom_off, tri_off, bytes; };
// bvh: the tree is walked (else the list: no LDS but the triangle counter's); global_nodes: RTW_FLAG_GLOBAL_NODES; geom: RenderNeed.geom;
// large: the request's NODES == 1 build is a large-workgroup one (bvh_block); triangles: the request has some.
// The layout: f16 nodes FIRST (LDS offset 0: the hottest address of the kernel, the node fetch of every visit, then needs no base register
// -- as the second block its offset was an SGPR the allocator spilled, one v_readlane per visit), then the per-lane stack (sentinel + one
// entry per tree level + the slot above the top the descend step always writes, at least four levels; 16-bit entries beside LDS nodes),
// then the optional sphere geometry: it rides along (NODES == 2) only while the workgroup stays under a sixth of the CU, i.e. while it does
// not cost a resident workgroup, or as RTW_OPT_LDS_GEOM says (n_spheres <= RTW_LDS_GEOM_MAX), never under RTW_OPT_NODE_FORMAT = 2.
// A large-workgroup build walks the tree as f32 planes, its stack's rows are RTW_BLOCK_LARGE entries, and it is meant to run two workgroups
// per CU (24 waves, 6 per SIMD).  Both fit the CU for every tree build_bvh gives f16 nodes within its depth cap: 3.5 x the node bytes + 3 x the
// stack bytes of a layout that fits a seventh.  A tree that does not fit (once, under RTW_OPT_NODE_FORMAT = 2), or RTW_OPT_NODE_FORMAT = 1,
// takes the f16 walk at RTW_BLOCK threads in the build that holds the spheres' geometry in LDS too (NODES == 2: a large build has no GEOM
// stage, and a tree with f16 nodes has at most RTW_LDS_GEOM_MAX spheres) -- whatever RTW_OPT_LDS_GEOM says.
LdsLayout render_lds_layout(const RtwTreeFacts &t, int opt_lds_geom, uint32_t opt_node_format, bool bvh, bool global_nodes, bool geom, bool large,
                            bool triangles);

// Host twin of the render kernel's closest-hit query over a built tree (a measuring and testing tool: the product traverses on the
// GPU).  Same order of events: the big list first, per-ray rho / tau, boxes inflated by rho, the f16 outward-rounded planes when the
// tree has them, the nearer child first (ties: child 0), pruning against best_t + tau; `node_visits` counts what RtwStats.node_tests
// counts.  The sphere test is a plain f32 quadratic with ties to the lower index, the same one `use_tree = false` walks the list with.
struct HostHit { int32_t sphere; float t; uint32_t node_visits, leaf_tests; };
HostHit bvh_closest_host(const BvhBuild &bb, const RtwSphere *spheres, uint32_t n, const float o[3], const float d[3], float time,
                         float mint, float maxt, bool use_tree, std::string *ops = nullptr);


// ---- queue order of the 8x8 tiles (RTW_OPT_TILE_ORDER) -------------------------------------------------------------------
// What the ordering heuristic may know about the scene: the spheres kept outside the tree (the ground) and the root box of
// the tree's spheres.  n_other != 0 (quads / instances present) switches the cheap-tile guess off.
struct SceneCull {
    float big[16][4];            // centre, radius
    uint32_t n_big = 0;
    uint32_t has_tree = 0;
    float lo[3] = { 0, 0, 0 }, hi[3] = { 0, 0, 0 };   // root box of the tree (time-expanded)
    uint32_t n_other = 0;
};
// fills has_tree / lo / hi from a built tree
void scene_cull_from_bvh(const BvhBuild &bb, const RtwSphere *spheres, SceneCull &out);
struct TileOrderKey {            // everything the order depends on (compared bytewise)
    uint32_t mode, tiles_x, tiles_y, k_base, row_block, part_index, part_count, scene_serial, tail_tiles;
    RtwCamera cam;
};
// mode 1: groups of 8 consecutive tiles scattered over the frame by a multiplicative bijection (waves then work on a mix of cheap and
//         expensive image regions at any time instead of all on the same band);
// mode 2: longest-processing-time-first by an estimated cost per tile (class of the tile's centre ray -- sphere field, ground only,
//         sky -- then distance, nearer first): the launch ends on its cheapest tiles;
// mode 3: reverse raster (bottom rows first).
// `order` receives a permutation of [0, tiles_x * tiles_y).  The image never depends on it.
void build_tile_order(uint32_t mode, uint32_t tiles_x, uint32_t tiles_y, uint32_t k_base, uint32_t row_block, uint32_t part_index,
                      uint32_t part_count, const RtwCamera &cam, const SceneCull &cull, uint32_t tail_tiles, std::vector<uint32_t> &order);

} // namespace rtw
