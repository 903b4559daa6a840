// rtw_shim.hip -- extern "C" entry points of librtw_hip.so (include/rtw.h): context, scene upload,
// blocking render.  Host code only; kernels live in rtw_kernels.hip.  No CPU fallback of any kind:
// without a HIP device every render entry point fails with RTW_E_NO_DEVICE / RTW_E_HIP.
#include "rtw_kernels.h"
#include "rtw_mesh.h"
#include "rtw_refit.h"
#include "rtw_host.h"
#include "rtw_filter.h"
#include "rtw_atrous_dev.h"
#include "rtw_temporal_dev.h"
#include "rtw_temporal.h"
#include "rtw_svgf_dev.h"
#include "rtw_bounds_dev.h"
#include "rtw_upsample_dev.h"
#include "rtw_display_dev.h"
#include "rtw_bloom_dev.h"
#include "rtw_devmem.h"
#include "rtw_exp.h"
#include "rtw_probe.h"
#include "rtw_ao.h"
#include "rtw_direct.h"

#include <link.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <new>
#include <utility>
#include <vector>

using namespace rtw;

static thread_local int g_last_hip = 0;

#define HIP_TRY(expr)                                                     \
    do {                                                                  \
        hipError_t e_ = (expr);                                           \
        if (e_ != hipSuccess) { g_last_hip = (int)e_; return RTW_E_HIP; } \
    } while (0)

// Every allocation of a context is a DevMem / PinnedMem (rtw_devmem.h) in one of these groups; a group is dropped as a unit by assigning an empty
// one.  The kernels never see them: they get the typed views (DevScene, DevGeom, DevBvh, DevTris, DevNoise) that rtw_ctx_set_* fill from the buffers.
struct SceneMem {
    DevMem geom, vel, mat, tex, texels;
    DevMem quads, inst, igeom, ivel, imat, iquads;
    DevMem nodes, nodes16, nodes32, big_geom, big_vel, big_index;
};
struct NoiseMem { DevMem perlin, tex_noise; };
struct TriMem {
    DevMem list, leaf, nodes;
    DevMem order, ouv, bad;              // the refit's (rtw_ctx_refit_triangles): its schedule, the staging of a host `ouv`, the count of refused triangles
};
#define REFIT_OUV_BYTES (9 * sizeof(float))      // one triangle of a refit's input: origin, u, v
#define REFIT_READBACK_BYTES 64u                 // u32 count at 0, TriNode at 32
struct QuatMem { DevMem rows; };
struct MeshMem {
    DevMem rows, top;                    // top: the top-level tree's nodes, the leaf-order placement indices behind them
    DevMem order, first, poses, counts;  // the move's (rtw_ctx_move_mesh_instances): the top-level tree's height schedule and its `first` on the device,
                                         // the staging of host poses, the counts of invalid poses and of placements beyond reach
};
#define MOVE_POSE_BYTES (7 * sizeof(float))      // one placement of a move's input: position, quaternion
// Buffers of rtw_ctx_mesh_instance_motion, grown on demand and kept until the context is destroyed: the staging of host poses and of rows for a
// host result, the count of refused poses and its pinned read-back.  A call on device buffers of a size seen before allocates nothing.
struct MotionMem { DevMem prev, cur, rows, bad; PinnedMem h_bad; };
// ... and of rtw_ctx_deform_motion: the staging of each host input and of each host result
struct DeformMem { DevMem tri, bary, ouv, idx, poses, point, normal; };
struct ScratchMem {
    DevMem queue, stats;
    PinnedMem h_stats;                   // pinned: the counter read-back is a true async copy
    PinnedMem h_refit;                   // a refit's read-back: the count of refused triangles, then node 0
    DevMem qstats; PinnedMem h_qstats;   // counters of the scene queries: RTW_QUERY_SLOTS lines of RTW_QUERY_STRIDE (rtw_kernels.h)
    DevMem out;                          // compact rows of a render whose destination the kernels cannot write
    PinnedMem h_out;                     // pinned staging for a multi-GPU frame in PAGEABLE host memory: a device-to-host copy into pageable memory returns only
                                         // when it is done, which would hold the fork of rtw_mgpu_render at this device until it has rendered its share
    DevMem order;                        // RTW_OPT_TILE_ORDER: queue position -> tile, valid for order_key
    DevMem samples;                      // per-sample radiance bank (see render_enqueue)
};

struct rtw_ctx {
    int device = 0;
    int n_cu = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_mark = nullptr;        // "the call began", recorded on this context's stream before anything of the call is launched anywhere (RtwStats.start_ms)
    // scene
    bool has_scene = false;
    bool has_textures = false;
    bool bvh_ok = true;                  // false: the tree is deeper than the device stack (never with build_bvh's invariant; checked anyway)
    double scene_span = 0.0;             // largest |coordinate| a sphere's centre reaches over [t_begin, t_end]; +inf when a centre, velocity or radius is not a number
                                         // or a centre / velocity is infinite (rtw_ctx_render: only ordinary scenes go through the tree)
    float t_begin = 0.0f, t_end = 0.0f;  // ray.time range the BVH bounds were expanded for (rtw_ctx_set_scene)
    DevScene sc{};
    float bg[3] = { 0, 0, 0 };
    DevGeom geom{};
    DevBvh bvh{};
    const uint32_t *nodes32 = nullptr;   // the f32 plane format of bvh.nodes16 (pack_nodes32), or null: no f16 nodes, or too many for its 16-bit codes
    SceneMem scene_mem;
    // texture noise of the scene (rtw_ctx_set_texture_noise; cleared by rtw_ctx_set_scene)
    uint32_t n_textures = 0;
    std::vector<uint8_t> tex_used;       // [n_textures]: a sphere, quad or instance member reads texture i
    bool noise_active = false;           // a used texture has noise: renders take the noise build (SPEC 7)
    DevNoise noise{};                    // device tables / per-texture entries (null when no noise is set)
    NoiseMem noise_mem;
    AtrousScratch *atrous = nullptr;     // buffers of rtw_ctx_atrous_filter (rtw_atrous.hip), rtw_ctx_svgf_filter and rtw_ctx_variance_estimate
                                         // (rtw_svgf.hip), created on the first call of any of them
    BoundsScratch *bounds = nullptr;     // buffers of rtw_ctx_colour_bounds (rtw_bounds.hip), created on its first call
    UpsampleScratch *upsample = nullptr; // buffers of rtw_ctx_upsample_filter (rtw_upsample.hip), created on its first call
    DisplayScratch *display = nullptr;   // buffers of rtw_ctx_luminance_histogram and rtw_ctx_display (rtw_display.hip), created on their first call
    BloomScratch *bloom = nullptr;       // buffers and pyramid of rtw_ctx_bloom (rtw_bloom.hip), created on its first call
    TemporalScratch *temporal = nullptr; // buffers of rtw_ctx_temporal_accumulate (rtw_temporal.hip), created on its first call
    FilterScratch *filter = nullptr;     // buffers of rtw_ctx_bilateral_filter (rtw_filter.hip), created on its first call
    MotionMem motion_mem;                // buffers of rtw_ctx_mesh_instance_motion
    DeformMem deform_mem;                // buffers of rtw_ctx_deform_motion
    // Rust2 triangles of the scene (rtw_ctx_set_triangles; cleared by rtw_ctx_set_scene)
    DevTris tris{};                      // tris.nodes stays null here: a render sets it (tri_view) when the tree may be used
    bool tri_tree = false;               // no triangle breaks the cull's derivation (DESIGN.md "Rust2 triangles")
    TriNode tri_root{};                  // the tree's root: the box every placement's world box is formed from (rtw_ctx_set_mesh_instances)
    TriMem tri_mem;
    bool tri_root_stale = false;         // a refit stopped half-way (a HIP error): tri_root no longer bounds the triangles; placements are refused until
                                         // a refit or rtw_ctx_set_triangles succeeds
    std::vector<uint32_t> refit_first;   // RefitSchedule.first of the tree in tri_mem (rtw_refit.h): the refit's launches
    // lights of the scene (rtw_ctx_set_lights; cleared by rtw_ctx_set_scene): the rows the light build reads from its arguments
    DevLights lights{};
    std::vector<DirectRow> light_rows;   // ... and their geometry as the direct-lighting pass reads it (rtw_direct.h), one row per light: its device table
                                         // is staged from here by every call of the pass
    std::vector<RtwSphere> h_spheres;    // host copies of the top-level spheres and quads: a light's mid-point is formed from them
    std::vector<RtwQuad> h_quads;
    bool has_medium = false;             // an instance of the scene is a constant-density medium (the light integrators refuse it)
    // Rust2's instance rotations (rtw_ctx_set_instance_rotations; cleared by rtw_ctx_set_scene): one normalised quaternion per instance
    std::vector<RtwInstance> h_instances;   // host copy of the instances: the checks of the setter read them
    const f4 *inst_quats = nullptr;      // non-null: renders take the quaternion build (SPEC 11), the queries rotate by them
    QuatMem quat_mem;
    // mesh placements (rtw_ctx_set_mesh_instances; cleared by rtw_ctx_set_scene and rtw_ctx_set_triangles): two rows per placement (rtw_mesh.h)
    const f4 *mesh_rows = nullptr;       // non-null: renders take the placement build (SPEC 12), the queries place the mesh
    uint32_t n_mesh = 0;
    const TriNode *mesh_top = nullptr;   // the top-level tree over the placements, or null: n < 2.  A render or query takes it
    uint32_t n_mesh_top = 0;             // through mesh_top_view
    bool mesh_top_ok = false;            // no placement lies beyond the reach of the tree's bound (and no move stopped half-way): the tree may be walked
    uint32_t n_top_nodes = 0;            // the nodes in mesh_mem.top (one leaf for n == 1, which no walk reads: the move's placement pass runs on it)
    std::vector<uint32_t> move_first;    // RefitSchedule.first of the top-level tree: the move's launches
    bool tri_textured = false;           // a triangle of the context reads an image texture (placements refuse such a mesh)
    MeshMem mesh_mem;
    // MixedMaterial (RTW_FLAG_MIXED_MATERIAL): does the scene hold an object with opacity < 0, and is the exponent (ir) of every such object
    // finite and >= 0?  Computed once by rtw_ctx_set_scene.
    bool has_mixed = false, mixed_bad = false;
    ScratchMem scr;
    TileOrderKey order_key{};
    SceneCull cull{};                    // what the tile-order heuristic knows about the scene (host copy, set by rtw_ctx_set_scene)
    uint32_t scene_serial = 0;           // bumped by every rtw_ctx_set_scene
    // options (rtw_ctx_set_option)
    uint32_t opt_chunk_len = 0;          // 0 = auto (render_enqueue); round 1 tuned a fixed 4 on the bench frame (1: 13.5, 2: 17.0, 4: 17.9, 8: 17.3, 16: 16.8 Gsegments/s)
    uint64_t opt_bank_bytes = 48ull << 30;
    int opt_lds_geom = -1;
    uint32_t opt_blocks_per_cu = 0;
    uint32_t opt_list_walk_max = RTW_LIST_WALK_MAX_DEFAULT;
    uint32_t opt_mesh_list_max = RTW_MESH_LIST_MAX_DEFAULT;   // RTW_OPT_MESH_LIST_MAX (profiles/mesh_top_tree.log)
    uint32_t opt_mesh_climb = 0;         // RTW_OPT_MESH_CLIMB: 0 = by node count (mesh_climb_one_group), 1 = one launch per height, 2 = one workgroup
    uint32_t opt_tile_order = 0;         // raster.  (The cost order, 2, was the default while units were 4 samples and grabs single blocks -- profiles/
                                         // r02_order_chunk_grid.log --; with today's units and grabs raster is 1.2 % ahead of it on the bench frame and ahead
                                         // on every other config too, profiles/r02_order_ab.log)
    uint32_t opt_sub_queues = 0;         // RTW_OPT_SUB_QUEUES: 0 = eight sub-queues (one per XCD) for all but tiny launches, 1 = a single queue
    double opt_tail_units = 0.0;         // RTW_OPT_TAIL_UNITS: blocks of short units per resident wave at the end of the queue (render_enqueue); 0 = off.
                                         // OFF by default: measured, it does not shorten a launch (profiles/r03_tail_units.log, r03_endtimes.log)
    uint32_t opt_guided_layout = 0;      // RTW_OPT_GUIDED_LAYOUT: where rtw_ctx_guided_filter keeps its table and guide tile (0 = by size)
    uint32_t opt_histogram_count = 0;    // RTW_OPT_HISTOGRAM_COUNT: how rtw_ctx_luminance_histogram keeps its LDS counts (0 = the measured choice)
    uint32_t opt_atrous_layout = 0;      // RTW_OPT_ATROUS_LAYOUT: where a level of rtw_ctx_atrous_filter reads its taps (0 = the measured choice)
    uint32_t opt_node_format = 0;        // RTW_OPT_NODE_FORMAT: 0 = f32 planes where a build walks them and two of its workgroups fit a CU's LDS, 1 = f16, 2 = f32
    uint32_t opt_grab_blocks = 2;        // RTW_OPT_GRAB_BLOCKS (profiles/r02_grab_sweep.log: 1 / 2 / 4 / 8 / a tile's 42 blocks = 83.9 / 82.9 / 83.7 / 86.8 / 107.9 ms on the bench frame)

    RenderBuild last_build{};            // the render kernel the last launch ran (rtw_ctx_last_render_build); every band of a render runs the same one
    bool has_last_build = false;
    uint32_t last_node_format = 0;       // ... and the LDS node format it read (rtw_ctx_last_node_format)
    std::vector<RtwQueuePlan> last_plans;   // ... and the work queue of each of its bands as launched (rtw_ctx_last_queue_plan)
    // cache of a per-call driver query (tens of microseconds: visible on small frames)
    std::map<const void *, uint32_t> lds_allowed;        // kernel -> the largest dynamic LDS it has been allowed beyond 64 KiB
    std::map<std::pair<const void *, uint32_t>, uint32_t> occupancy;    // (kernel, dynamic LDS bytes) -> resident workgroups per CU
    bool attr_on_device = false; int attr_device = -1;   // memory kind of this call's out_rgb
    // the render in flight between render_enqueue and render_wait
    struct Pending {
        bool active = false;
        bool marked = false;             // ev_mark was recorded for this call (by rtw_mgpu_render, before any device was given work)
        uint32_t n_rows = 0;
        std::chrono::steady_clock::time_point t0;      // the call's begin on the host (rtw_mgpu_render: the same instant for every device)
        float enqueue_ms = 0.0f;         // host time from t0 until this context's launches had been issued
        // where the rendered rows go (render_copy / render_wait)
        float *dst = nullptr; bool scatter = false, direct = false, staged = false;
        uint32_t width = 0, height = 0, row_block = 1, part_index = 0, part_count = 1;
        size_t out_bytes = 0;
    } pend;
};

// Where a render's rows go.
struct OutSpec {
    float *base;        // compact [rows][width][3] buffer, or -- scatter -- the full [height][width][3] frame
    bool scatter;       // copy every row block to its image rows of the full frame (multi-GPU: no gather buffer, no de-interleave pass)
};

// The device records of a sphere list (sphere.rs:13-20 + materials.rs:15-20)
static void prepare_spheres(const RtwSphere *sp, uint32_t n, const RtwTexture *tex, std::vector<f4> &geom, std::vector<f4> &vel, std::vector<DevMat> &mat, bool &moving) {
    geom.resize(n); vel.resize(n); mat.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        const RtwSphere &s = sp[i];
        geom[i] = f4{ s.center[0], s.center[1], s.center[2], host_mul(s.radius, s.radius) };   // sphere.rs:105 radius*radius
        vel[i] = f4{ s.velocity[0], s.velocity[1], s.velocity[2], 0.0f };
        if (s.velocity[0] != 0.0f || s.velocity[1] != 0.0f || s.velocity[2] != 0.0f) moving = true;
        DevMat &m = mat[i];
        std::memset(&m, 0, sizeof m);
        for (int k = 0; k < 3; k++) {
            // tex < 0: (texel * 1.0) * col_mod hoisted (texture.rs:265, sphere.rs:145)
            m.cm[k] = s.tex < 0 ? host_mul(host_mul(s.tex_color[k], 1.0f), s.col_mod[k]) : s.col_mod[k];
            m.emitted[k] = s.emitted[k];
        }
        m.metallicness = s.metallicness; m.opacity = s.opacity; m.ir = s.ir; m.tex = s.tex;
        // the image's shape and place ride along in the material record: the texel fetch then depends on ONE load (this record), not on a second one
        // of the RtwTexture behind it (a SHADE step of a textured scene was three dependent global loads deep: material -> texture -> texel)
        if (s.tex >= 0 && tex) { m.tex_row = tex[s.tex].row; m.tex_col = tex[s.tex].col; m.tex_offset = tex[s.tex].texel_offset; }
        m.inv_ir = host_div(1.0f, s.ir);                         // materials.rs:113  1.0 / self.ir
        m.r0_front = schlick_r0(m.inv_ir); m.r0_back = schlick_r0(s.ir);   // materials.rs:99-100 for either ratio
    }
}

// Quad::new (quad.rs:84-110): n = u x v, normal = unit(n), d = normal . origin, w = n / (n . n) -- one rounding per
// written operation (this TU is built with -ffp-contract=off), the oracle computes the same independently.
static void prepare_quads(const RtwQuad *q, uint32_t n, std::vector<DevQuad> &out) {
    out.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        const RtwQuad &s = q[i];
        DevQuad &d = out[i];
        std::memset(&d, 0, sizeof d);
        const float nx = s.u[1] * s.v[2] - s.u[2] * s.v[1], ny = s.u[2] * s.v[0] - s.u[0] * s.v[2], nz = s.u[0] * s.v[1] - s.u[1] * s.v[0];
        const float len = std::sqrt(nx * nx + ny * ny + nz * nz);
        d.normal[0] = nx / len; d.normal[1] = ny / len; d.normal[2] = nz / len;
        d.d = d.normal[0] * s.origin[0] + d.normal[1] * s.origin[1] + d.normal[2] * s.origin[2];
        const float nn = nx * nx + ny * ny + nz * nz;
        d.w[0] = nx / nn; d.w[1] = ny / nn; d.w[2] = nz / nn;
        for (int k = 0; k < 3; k++) {
            d.origin[k] = s.origin[k]; d.u[k] = s.u[k]; d.v[k] = s.v[k];
            d.albedo[k] = host_mul(s.tex_color[k], 1.0f);            // texture.rs:265
            d.emitted[k] = s.emitted[k];
        }
        d.metallicness = s.metallicness; d.opacity = s.opacity; d.ir = s.ir; d.tex = s.tex;
    }
}

template <class T>
static int upload(DevMem &dst, const std::vector<T> &src) {
    HIP_TRY(dst.reserve(src.empty() ? sizeof(T) : src.size() * sizeof(T)));       // (an empty list is still an address: "absent" is the caller's decision)
    if (!src.empty()) HIP_TRY(hipMemcpy(dst.ptr, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return RTW_OK;
}

// How many copies of the HIP runtime are mapped into this process.  librtw_hip.so links /opt/rocm's libamdhip64; PyTorch ships its own.  When torch
// is imported FIRST the dynamic linker gives this library the copy that is already loaded (same soname) and all is well; when this library is
// loaded first, a later `import torch` brings up a SECOND runtime whose device enumeration fails ("No HIP GPUs are available",
// gpurun_out/r02_debug_torch.log) -- torch is then blind for the rest of the process.  A context created in such a process fails loudly instead.
static int count_hip_runtimes_cb(struct dl_phdr_info *info, size_t, void *data) {
    if (info->dlpi_name && std::strstr(info->dlpi_name, "libamdhip64")) ++*(int *)data;
    return 0;
}

// ---- what the calls that stage and the scene query passes share ----------------------------------------------------------------------
// The end of a call that works through temporaries of its own (a Staging): `e` is what its chain of HIP calls came to.  After a failure the
// stream is waited for first -- part of the chain may have been enqueued, and nothing may still use the temporaries when the caller's scope frees them.
static int call_status(rtw_ctx *c, hipError_t e) {
    if (e == hipSuccess) return RTW_OK;
    (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
    g_last_hip = (int)e;
    return e == hipErrorOutOfMemory ? RTW_E_NOMEM : RTW_E_HIP;
}

// The caller pointers of one call, as addresses this context's kernels can use: the caller's own where it is this GPU's memory (on_device, asked
// once per pointer), else a temporary -- always one with `always` (the calls whose documented arrays are host arrays).  Everything is enqueued on
// c->stream, so an input is read behind the caller's producers; `e` is the call's chain of HIP results, and after a failure nothing more is
// enqueued.  The temporaries live as long as the object: declare it in the entry point, so that they die after call_status has run.
struct Staging {
    hipError_t e = hipSuccess;

    explicit Staging(rtw_ctx *ctx, bool always_stage = false) : c(ctx), always(always_stage) {}
    // a temporary of `bytes` that nobody gets back
    template <class T = void> T *scratch(size_t bytes) {
        if (n_tmp == MAX) { if (e == hipSuccess) e = hipErrorInvalidValue; return nullptr; }
        DevMem &m = tmp[n_tmp++];
        if (e == hipSuccess) e = m.reserve(bytes);
        return m.as<T>();
    }
    // an input of `bytes`: a temporary gets the copy in enqueued
    template <class T> const T *in(const T *p, size_t bytes) {
        if (!always && on_device(p, c->device)) return p;
        T *d = scratch<T>(bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(d, p, bytes, hipMemcpyDefault, c->stream);
        return d;
    }
    // an output of `bytes`: a temporary is noted for copy_out
    template <class T> T *out(T *p, size_t bytes) {
        if (!always && on_device(p, c->device)) return p;
        T *d = scratch<T>(bytes);
        if (d) back[n_back++] = { p, d, bytes };
        return d;
    }
    // enqueue the copies of all staged outputs to their callers, in the order they were asked for
    hipError_t copy_out() {
        for (int i = 0; i < n_back; i++)
            if (e == hipSuccess) e = hipMemcpyAsync(back[i].dst, back[i].src, back[i].bytes, hipMemcpyDefault, c->stream);
        return e;
    }
    // the end of a call without counters: the copies out, the call's one synchronise, its status
    int finish() {
        if (copy_out() == hipSuccess) e = hipStreamSynchronize(c->stream);
        return call_status(c, e);
    }

private:
    static constexpr int MAX = 9;        // (rtw_ctx_scene_surface_tri stages nine)
    struct Back { void *dst; const void *src; size_t bytes; };
    rtw_ctx *c;
    bool always;
    DevMem tmp[MAX];
    Back back[MAX];
    int n_tmp = 0, n_back = 0;
};

// The triangle view a render or query of this context uses: the tree only for RTW_ACCEL_BVH and a range the cull's derivation covers
static DevTris tri_view(const rtw_ctx *c, uint32_t accel, float mint, float maxt) {
    DevTris t = c->tris;
    const float tb = std::fmax(std::fabs(mint), std::fabs(maxt));
    t.t_bound = tb;
    const bool range_ok = std::isfinite(mint) && std::isfinite(maxt) && tb <= RTW_TRI_COORD_MAX;
    t.nodes = (accel == RTW_ACCEL_BVH && c->tri_tree && range_ok) ? c->tri_mem.nodes.as<TriNode>() : nullptr;
    return t;
}

// ... and the top-level tree over its placements: only next to the mesh's own tree (T = tri_view's answer: RTW_ACCEL_BVH, a mesh and a range
// the cull covers), for more than RTW_OPT_MESH_LIST_MAX placements and while none of them lies beyond the reach of the tree's bound; else null,
// and the placements are met in list order (the same answer)
static const TriNode *mesh_top_view(const rtw_ctx *c, const DevTris &T) {
    return (T.nodes != nullptr && c->n_mesh > c->opt_mesh_list_max && c->mesh_top_ok) ? c->mesh_top : nullptr;
}

// Does a query's sphere group go through the tree?  The conditions a render puts on it (render_enqueue_impl); the per-ray ones are checked by
// the kernels, ray by ray.  ONE definition for the closest-hit and the any-hit query: rtw_ctx_scene_occluded's contract is stated against
// rtw_ctx_scene_hits with the same arguments.
static bool query_uses_tree(const rtw_ctx *c, uint32_t accel, float time, float mint, float maxt) {
    bool tree = accel == RTW_ACCEL_BVH && c->bvh_ok && c->sc.n > c->opt_list_walk_max;
    if (mint != mint || maxt != maxt || time != time) tree = false;
    if (!(c->scene_span <= 1e18)) tree = false;
    if (c->sc.moving && !(time >= c->t_begin && time <= c->t_end)) tree = false;
    return tree;
}

// The scene views, the range and the counters of a launch over n rays or points: everything QueryArgs and OccludedArgs share by name, the rest
// zero.  ONE definition for the closest-hit, the any-hit and the AO kernels, so that they walk the same groups through the same trees.
template <class A>
static void scene_views(const rtw_ctx *c, uint32_t n, float time, float mint, float maxt, uint32_t accel, A &q) {
    std::memset(&q, 0, sizeof q);
    q.sc = c->sc; q.bvh = c->bvh; q.geom = c->geom; q.inst_quats = c->inst_quats;
    if (c->tris.n) q.tris = tri_view(c, accel, mint, maxt);
    q.mesh_rows = c->mesh_rows; q.n_mesh = c->n_mesh;
    if (c->mesh_rows) { q.mesh_top = mesh_top_view(c, q.tris); q.n_mesh_top = c->n_mesh_top; }
    q.n = n; q.levels = c->bvh.depth + 2u;
    q.time = time; q.mint = mint; q.maxt = maxt; q.span = (float)c->scene_span;
    q.counters = c->scr.qstats.as<unsigned long long>();
}

// The frame of a pass that counts (scr.qstats), on c->stream: the counters zeroed, ev0, each of `launch` in turn, ev1, the staged outputs to
// their callers, the counters to scr.h_qstats, the call's one synchronise; then the counter lines (RTW_QUERY_SLOTS) summed into `stats` with
// segments = `samples` per point that cast rays (counter 4) + `extra`.  RTW_E_INTERNAL when a wave's stack was too short (counter 3).
template <class... Launch>
static int counted_pass(rtw_ctx *c, Staging &st, uint32_t samples, uint64_t extra, RtwStats *stats, Launch &&...launch) {
    const size_t q_bytes = RTW_QUERY_SLOTS * RTW_QUERY_STRIDE * sizeof(unsigned long long);
    hipError_t &e = st.e;
    if (e == hipSuccess) e = hipMemsetAsync(c->scr.qstats.ptr, 0, q_bytes, c->stream);
    if (e == hipSuccess) e = hipEventRecord(c->ev0, c->stream);
    const auto run = [&e](auto &one) { if (e == hipSuccess) { one(); e = hipGetLastError(); } };
    (run(launch), ...);
    if (e == hipSuccess) e = hipEventRecord(c->ev1, c->stream);
    if (st.copy_out() == hipSuccess) e = hipMemcpyAsync(c->scr.h_qstats.ptr, c->scr.qstats.ptr, q_bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev0, c->ev1);
    if (const int rc = call_status(c, e)) return rc;
    const unsigned long long *h_qstats = c->scr.h_qstats.as<unsigned long long>();
    unsigned long long sum[5] = { 0, 0, 0, 0, 0 };
    for (uint32_t s = 0; s < RTW_QUERY_SLOTS; s++) for (int k = 0; k < 5; k++) sum[k] += h_qstats[s * RTW_QUERY_STRIDE + k];
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->segments = sum[4] * samples + extra;
        stats->sphere_tests = sum[0]; stats->node_tests = sum[1]; stats->quad_tests = sum[2];
        stats->kernel_ms = ms;
    }
    return sum[3] ? RTW_E_INTERNAL : RTW_OK;
}

// ---- what the fused passes (ambient occlusion, direct lighting; kernels: rtw_occluded.hip) share on top of it ---------------------------
// A fused launch over n points: everything zero, a.q the scene_views of the points and the range of its rays, and the sampling fields.
// A: AoArgs or DirectArgs, which name these fields alike.
template <class A>
static void fused_args(const rtw_ctx *c, uint32_t n, uint32_t samples, uint32_t seed, float time, float mint, float maxt, uint32_t accel, A &a) {
    std::memset(&a, 0, sizeof a);
    scene_views(c, n, time, mint, maxt, accel, a.q);
    a.samples = samples; a.seed = seed;
    while ((1u << a.lg_group) < samples && a.lg_group < 6u) a.lg_group++;
}

// The depth pass of a map call -- rtw_ctx_depth_map's launch with ids and normals -- and the buffers it hands to the pass behind it: each of
// the three outputs is the caller's where it was asked for (staged like any output) and scratch where not, and `src` reads all three for the
// same camera.  The two launches then run on the context's stream between one pair of events, with one set of counters.
template <class A>
static QueryArgs depth_pass(const rtw_ctx *c, Staging &st, const RtwCamera *cam, uint32_t width, uint32_t height, float time, float mint, float maxt,
                            uint32_t accel, float *depth_out, int32_t *idx_out, float *normal_out, A &src) {
    const uint32_t n = width * height;
    QueryArgs q;
    scene_views(c, n, time, mint, maxt, accel, q);
    src.cam = q.cam = *cam; src.width = q.width = width; src.height = q.height = height;
    q.miss_t = host_mul(maxt, 1.6f);
    const size_t t_bytes = sizeof(float) * (size_t)n, i_bytes = sizeof(int32_t) * (size_t)n;
    src.depth = q.t_out = depth_out ? st.out(depth_out, t_bytes) : st.scratch<float>(t_bytes);
    src.idx = q.idx_out = idx_out ? st.out(idx_out, i_bytes) : st.scratch<int32_t>(i_bytes);
    src.normals = q.normal_out = normal_out ? st.out(normal_out, 3 * t_bytes) : st.scratch<float>(3 * t_bytes);
    return q;
}

extern "C" {

int rtw_abi_version(void) { return RTW_ABI_VERSION; }

int rtw_hip_runtime_count(void) {
    int n = 0;
    dl_iterate_phdr(count_hip_runtimes_cb, &n);
    return n;
}

int rtw_last_hip_error(void) { return g_last_hip; }

int rtw_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *rtw_strerror(int status) {
    switch (status) {
    case RTW_OK: return "ok";
    case RTW_E_INVALID: return "invalid argument";
    case RTW_E_NO_DEVICE: return "no HIP device";
    case RTW_E_HIP: return "HIP runtime error";
    case RTW_E_NOMEM: return "out of memory";
    case RTW_E_UNSUPPORTED: return "not implemented on the device";
    case RTW_E_NO_SCENE: return "no scene set";
    case RTW_E_INTERNAL: return "a render kernel gave up (internal error): the image is incomplete";
    case RTW_E_RUNTIME_CONFLICT: return "two copies of the HIP runtime (libamdhip64) are loaded in this process -- typically PyTorch imported AFTER the first rtw_* call: "
                                        "import torch before using this library (the runtimes then share one copy), or link both against the same runtime";
    default: return "unknown status";
    }
}

int rtw_ctx_create(int device, rtw_ctx **out) {
    if (!out) return RTW_E_INVALID;
    *out = nullptr;
    if (rtw_hip_runtime_count() > 1) return RTW_E_RUNTIME_CONFLICT;
    int n = rtw_device_count();
    if (n <= 0 || device < 0 || device >= n) return RTW_E_NO_DEVICE;
    rtw_ctx *c = new (std::nothrow) rtw_ctx();
    if (!c) return RTW_E_NOMEM;
    c->device = device;
    hipError_t e = hipSetDevice(device);
    hipDeviceProp_t prop;
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) { c->n_cu = prop.multiProcessorCount; e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking); }
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e == hipSuccess) e = hipEventCreate(&c->ev_mark);
    if (e == hipSuccess) e = c->scr.queue.reserve(RTW_QUEUE_BYTES);
    if (e == hipSuccess) e = c->scr.stats.reserve(RTW_N_STATS * sizeof(unsigned long long));
    if (e == hipSuccess) e = c->scr.h_stats.reserve(RTW_N_STATS * sizeof(unsigned long long));
    if (e == hipSuccess) e = c->scr.qstats.reserve(RTW_QUERY_SLOTS * RTW_QUERY_STRIDE * sizeof(unsigned long long));
    if (e == hipSuccess) e = c->scr.h_qstats.reserve(RTW_QUERY_SLOTS * RTW_QUERY_STRIDE * sizeof(unsigned long long));
    if (e != hipSuccess) { g_last_hip = (int)e; rtw_ctx_destroy(c); return RTW_E_HIP; }
    c->stream = c->own_stream;
    *out = c;
    return RTW_OK;
}

static void free_noise(rtw_ctx *c) {
    c->noise_mem = NoiseMem{};
    c->noise = DevNoise{};
    c->noise_active = false;
}

static void free_mesh(rtw_ctx *c) {
    c->mesh_mem = MeshMem{};
    c->mesh_rows = nullptr;
    c->n_mesh = 0;
    c->mesh_top = nullptr;
    c->n_mesh_top = 0;
    c->mesh_top_ok = false;
    c->n_top_nodes = 0;
    c->move_first.clear();
}

static void free_tris(rtw_ctx *c) {
    free_mesh(c);                        // (placements are placements of these triangles)
    c->tri_textured = false;
    c->tri_mem = TriMem{};
    c->refit_first.clear();
    c->tri_root_stale = false;
    c->tris = DevTris{};
    c->tri_tree = false;
}

static void free_quats(rtw_ctx *c) {
    c->quat_mem = QuatMem{};
    c->inst_quats = nullptr;
}

static void free_scene(rtw_ctx *c) {
    c->scene_mem = SceneMem{};
    free_noise(c);
    free_tris(c);
    free_quats(c);
    c->h_instances.clear();
    c->lights = DevLights{};
    c->light_rows.clear();
    c->h_spheres.clear(); c->h_quads.clear(); c->has_medium = false;
    c->has_mixed = c->mixed_bad = false;
    c->n_textures = 0;
    c->tex_used.clear();
    c->has_scene = false;
}

void rtw_ctx_destroy(rtw_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    free_scene(c);                       // memory first, on its device, then the events and the stream: nothing is left for `delete` to free
    c->scr = ScratchMem{};
    filter_scratch_free(c->filter);
    atrous_scratch_free(c->atrous);
    temporal_scratch_free(c->temporal);
    bounds_scratch_free(c->bounds);
    upsample_scratch_free(c->upsample);
    display_scratch_free(c->display);
    bloom_scratch_free(c->bloom);
    if (c->ev_mark) (void)hipEventDestroy(c->ev_mark);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int rtw_ctx_set_stream(rtw_ctx *c, void *hip_stream) {
    if (!c) return RTW_E_INVALID;
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return RTW_OK;
}

// ---- MixedMaterial (rtw.h "MixedMaterial") ------------------------------------------------------------------------------------------
// Which objects of a scene RTW_FLAG_MIXED_MATERIAL turns into MixedMaterial::new(ir) -- opacity < 0, wherever {metallicness, opacity, ir} is
// carried -- and whether an exponent among them is outside pow_plain's domain (not finite, or negative).
static void scene_mixed(const RtwScene *s, bool &has_mixed, bool &mixed_bad) {
    has_mixed = mixed_bad = false;
    auto see = [&](float opacity, float ir) {
        if (!(opacity < 0.0f)) return;
        has_mixed = true;
        if (!(ir >= 0.0f && ir <= 3.402823466e38f)) mixed_bad = true;
    };
    for (uint32_t i = 0; i < s->n_spheres; i++) see(s->spheres[i].opacity, s->spheres[i].ir);
    for (uint32_t i = 0; i < s->n_quads; i++) see(s->quads[i].opacity, s->quads[i].ir);
    for (uint32_t i = 0; i < s->n_inst_spheres; i++) see(s->inst_spheres[i].opacity, s->inst_spheres[i].ir);
    for (uint32_t i = 0; i < s->n_inst_quads; i++) see(s->inst_quads[i].opacity, s->inst_quads[i].ir);
}
// What a render answers to RTW_FLAG_MIXED_MATERIAL: shared by rtw_ctx_render and rtw_mixed_validate (host only).
static int mixed_check(uint32_t flags, uint32_t integrator, bool has_mixed, bool mixed_bad, bool noise, bool tris, bool medium) {
    if (!(flags & RTW_FLAG_MIXED_MATERIAL)) return RTW_OK;
    if (integrator != RTW_INTEGRATOR_RUST2 && integrator != RTW_INTEGRATOR_LIGHT_CAST && integrator != RTW_INTEGRATOR_LIGHT_BIASED) return RTW_E_UNSUPPORTED;
    if (!has_mixed) return RTW_OK;
    if (mixed_bad) return RTW_E_INVALID;
    if (noise || tris || medium) return RTW_E_UNSUPPORTED;
    return RTW_OK;
}

int rtw_mixed_validate(const RtwScene *scene, const RtwParams *params, uint32_t n_triangles, uint32_t texture_noise) {
    if (!scene || !params) return RTW_E_INVALID;
    if ((scene->n_spheres && !scene->spheres) || (scene->n_quads && !scene->quads) || (scene->n_inst_spheres && !scene->inst_spheres) ||
        (scene->n_inst_quads && !scene->inst_quads) || (scene->n_instances && !scene->instances)) return RTW_E_INVALID;
    bool has_mixed, mixed_bad, medium = false;
    scene_mixed(scene, has_mixed, mixed_bad);
    for (uint32_t i = 0; i < scene->n_instances; i++) if (scene->instances[i].medium == RTW_MEDIUM_CONST_DENSITY) medium = true;
    return mixed_check(params->flags, params->integrator, has_mixed, mixed_bad, texture_noise != 0u, n_triangles != 0u, medium);
}

int rtw_mixed_dir(float exp, float xi_phi, float xi_cos, const float n[3], float out_dir[3]) {
    if (!n || !out_dir) return RTW_E_INVALID;
    const lv3 d = mixed_dir(exp, xi_phi, xi_cos, lmk(n[0], n[1], n[2]));
    out_dir[0] = d.x; out_dir[1] = d.y; out_dir[2] = d.z;
    return RTW_OK;
}

int rtw_mixed_pdf(float exp, const float p[3], const float n[3], const float dir_in[3], const float ray_o[3], const float ray_d[3], float *out) {
    if (!p || !n || !dir_in || !ray_o || !ray_d || !out) return RTW_E_INVALID;
    *out = mixed_pdf(exp, lmk(p[0], p[1], p[2]), lmk(n[0], n[1], n[2]), lmk(dir_in[0], dir_in[1], dir_in[2]), lmk(ray_o[0], ray_o[1], ray_o[2]),
                     lmk(ray_d[0], ray_d[1], ray_d[2]));
    return RTW_OK;
}

int rtw_pow_plain(const float *x, const float *y, size_t n, float *out) {
    if (n && (!x || !y || !out)) return RTW_E_INVALID;
    for (size_t i = 0; i < n; i++) out[i] = pow_plain(x[i], y[i]);
    return RTW_OK;
}
int rtw_exp_plain(const float *x, size_t n, float *out) {
    if (n && (!x || !out)) return RTW_E_INVALID;
    for (size_t i = 0; i < n; i++) out[i] = exp_plain(x[i]);
    return RTW_OK;
}
int rtw_sin_plain(const float *phi, size_t n, float *out) {
    if (n && (!phi || !out)) return RTW_E_INVALID;
    for (size_t i = 0; i < n; i++) out[i] = sin_plain(phi[i]);
    return RTW_OK;
}
int rtw_cos_plain(const float *phi, size_t n, float *out) {
    if (n && (!phi || !out)) return RTW_E_INVALID;
    for (size_t i = 0; i < n; i++) out[i] = cos_plain(phi[i]);
    return RTW_OK;
}

int rtw_ctx_set_scene(rtw_ctx *c, const RtwScene *s, float t_begin, float t_end) {
    if (!c || !s || (s->n_spheres && !s->spheres)) return RTW_E_INVALID;
    if ((s->n_textures && !s->textures) || (s->n_texels && !s->texels)) return RTW_E_INVALID;
    if ((s->n_quads && !s->quads) || (s->n_instances && !s->instances)) return RTW_E_INVALID;
    if ((s->n_inst_spheres && !s->inst_spheres) || (s->n_inst_quads && !s->inst_quads)) return RTW_E_INVALID;
    for (uint32_t i = 0; i < s->n_spheres; i++)
        if (s->spheres[i].tex >= (int32_t)s->n_textures) return RTW_E_INVALID;
    for (uint32_t i = 0; i < s->n_inst_spheres; i++)
        if (s->inst_spheres[i].tex >= (int32_t)s->n_textures) return RTW_E_INVALID;
    for (uint32_t i = 0; i < s->n_quads; i++)
        if (s->quads[i].tex >= (int32_t)s->n_textures) return RTW_E_INVALID;
    for (uint32_t i = 0; i < s->n_inst_quads; i++)
        if (s->inst_quads[i].tex >= (int32_t)s->n_textures) return RTW_E_INVALID;
    for (uint32_t i = 0; i < s->n_instances; i++) {
        const RtwInstance &in = s->instances[i];
        if ((uint64_t)in.first_sphere + in.n_spheres > s->n_inst_spheres) return RTW_E_INVALID;
        if ((uint64_t)in.first_quad + in.n_quads > s->n_inst_quads) return RTW_E_INVALID;
        if (in.medium > RTW_MEDIUM_CONST_DENSITY) return RTW_E_INVALID;
    }
    for (uint32_t i = 0; i < s->n_textures; i++) {
        const RtwTexture &t = s->textures[i];
        if (t.row == 0 || t.col == 0 || (uint64_t)t.texel_offset + (uint64_t)t.row * t.col > s->n_texels) return RTW_E_INVALID;
        if (t.emit_tex > s->n_textures) return RTW_E_INVALID;        // 1 + index of Rust2's emission image, 0 = none
    }
    HIP_TRY(hipSetDevice(c->device));
    free_scene(c);

    std::vector<f4> geom, vel;
    std::vector<DevMat> mat;
    bool moving = false;
    prepare_spheres(s->spheres, s->n_spheres, s->textures, geom, vel, mat, moving);
    std::vector<RtwTexture> tex(s->textures, s->textures + s->n_textures);
    std::vector<float> texels(s->texels, s->texels + 3 * (size_t)s->n_texels);

    SceneMem m;                          // the context gets it when all of it is there: a failure below leaves the context without a scene
    int rc;
    if ((rc = upload(m.geom, geom)) || (rc = upload(m.vel, vel)) || (rc = upload(m.mat, mat)) ||
        (rc = upload(m.tex, tex)) || (rc = upload(m.texels, texels))) return rc;

    // quads and instances (Scene::new, viewport.rs:122-135).  Their AABB trees (qaabb.rs, iaabb.rs) only prune list
    // walks over a handful of objects: the device walks the lists.
    {
        std::vector<DevQuad> quads, iquads;
        std::vector<f4> igeom, ivel; std::vector<DevMat> imat;
        std::vector<DevInstance> inst(s->n_instances);
        bool imoving = false;
        prepare_quads(s->quads, s->n_quads, quads);
        prepare_quads(s->inst_quads, s->n_inst_quads, iquads);
        prepare_spheres(s->inst_spheres, s->n_inst_spheres, s->textures, igeom, ivel, imat, imoving);
        for (uint32_t i = 0; i < s->n_instances; i++) {
            const RtwInstance &in = s->instances[i];
            DevInstance &d = inst[i];
            std::memset(&d, 0, sizeof d);
            d.first_sphere = in.first_sphere; d.n_spheres = in.n_spheres; d.first_quad = in.first_quad; d.n_quads = in.n_quads;
            d.density = in.density; d.medium = in.medium;
            for (int k = 0; k < 3; k++) {
                d.tr[k] = in.translation[k];
                d.back[2 * k] = std::sin(-in.rotation[k]); d.back[2 * k + 1] = std::cos(-in.rotation[k]);   // rotated(-self.rotation) (instance.rs:258)
                d.fwd[2 * k] = std::sin(in.rotation[k]);   d.fwd[2 * k + 1] = std::cos(in.rotation[k]);     // vec3.rs:163-170
            }
            rotation_coefficients(d.back, d.back_k); rotation_coefficients(d.fwd, d.fwd_k);
        }
        if ((rc = upload(m.quads, quads)) || (rc = upload(m.iquads, iquads)) || (rc = upload(m.inst, inst)) ||
            (rc = upload(m.igeom, igeom)) || (rc = upload(m.ivel, ivel)) || (rc = upload(m.imat, imat))) return rc;
        c->geom.quads = m.quads.as<DevQuad>(); c->geom.iquads = m.iquads.as<DevQuad>();
        c->geom.inst = m.inst.as<DevInstance>();
        c->geom.igeom = m.igeom.as<f4>(); c->geom.ivel = m.ivel.as<f4>(); c->geom.imat = m.imat.as<DevMat>();
        c->geom.n_quads = s->n_quads; c->geom.n_inst = s->n_instances;
    }

    // acceleration structure (Scene::new_sphere builds the AABB tree, viewport.rs:90-105)
    BvhBuild bb;
    build_bvh(s->spheres, s->n_spheres, std::fmin(t_begin, t_end), std::fmax(t_begin, t_end), bb);
    std::vector<f4> big_geom, big_vel;
    for (uint32_t i : bb.big) { big_geom.push_back(geom[i]); big_vel.push_back(vel[i]); }
    std::vector<uint32_t> nodes32;
    if (bb.nodes16.size() <= RTW_NODE32_NODES_MAX) pack_nodes32(bb.nodes16, nodes32);
    if ((rc = upload(m.nodes32, nodes32))) return rc;
    c->nodes32 = nodes32.empty() ? nullptr : m.nodes32.as<uint32_t>();
    if ((rc = upload(m.nodes16, bb.nodes16)) || (rc = upload(m.nodes, bb.nodes)) || (rc = upload(m.big_geom, big_geom)) ||
        (rc = upload(m.big_vel, big_vel)) || (rc = upload(m.big_index, bb.big))) return rc;
    c->bvh.nodes16 = bb.nodes16.empty() ? nullptr : m.nodes16.as<BvhNode16>();     // (null = "this tree has no f16 nodes": the kernels' builds differ)
    c->bvh.n_nodes = (uint32_t)bb.nodes.size();
    c->bvh.nodes = m.nodes.as<BvhNode>();
    c->bvh.big_geom = m.big_geom.as<f4>(); c->bvh.big_vel = m.big_vel.as<f4>();
    c->bvh.big_index = m.big_index.as<uint32_t>(); c->bvh.n_big = (uint32_t)bb.big.size();
    c->bvh.root = bb.root; c->bvh.depth = bb.depth;
    c->bvh_ok = bb.depth <= RTW_BVH_STACK;        // build_bvh guarantees it; a deeper tree would overflow the per-lane LDS stack
    {   // The tree prunes on the premise that the reference's quadratic is computed in ORDINARY f32 (DESIGN.md "Conservative traversal").  A centre at 1e19 or
        // beyond (|oc|^2 overflows), or a NaN anywhere, makes its discriminant NaN, and a NaN root passes both range tests of sphere.rs:118-121: such a sphere is
        // "hit" by every ray that reaches it in list order with nothing accepted before -- an order-dependent answer only the list walk gives.  Record how far the
        // centres reach; rtw_ctx_render decides with the camera in hand.  (Radii: +-inf and huge ones are fine -- those spheres are tested exactly for every
        // query, and r^2 = inf gives -inf / +inf roots, no NaN; a NaN radius is not.)
        double span = 0.0;
        const double tmax = std::fmax(std::fabs((double)t_begin), std::fabs((double)t_end));
        for (uint32_t i = 0; i < s->n_spheres; i++) {
            const RtwSphere &q = s->spheres[i];
            double reach = 0.0;
            bool odd = q.radius != q.radius;
            // ... and a material that can turn a ray into one: the scattered direction is reflect * m + scatter * (1 - m), or a refraction with ratio ir or 1 / ir
            // (materials.rs:105-154) -- finite and of ordinary size exactly when m and ir are (a NaN or 1e30 there makes the NEXT ray NaN or |d|^2 overflow)
            {
                const double m = std::fabs((double)q.metallicness), ir = std::fabs((double)q.ir);
                if (!(m <= 1e10)) odd = true;
                if (q.opacity > 0.0f && !(ir >= 1e-10 && ir <= 1e10)) odd = true;         // (ir is read by the dielectric branch only)
            }
            for (int k = 0; k < 3; k++) {
                const double a = std::fabs((double)q.center[k]), v = std::fabs((double)q.velocity[k]);
                if (!(a <= 1.7e308) || !(v <= 1.7e308)) odd = true;                   // NaN or inf (NaN compares false: the negated tests catch it; fmax would drop it)
                else reach = std::fmax(reach, a + v * tmax);
            }
            span = std::fmax(span, odd ? HUGE_VAL : reach);
        }
        c->scene_span = span;
    }
    c->scene_serial++;
    scene_cull_from_bvh(bb, s->spheres, c->cull);
    c->cull.n_other = s->n_quads + s->n_instances;
    c->t_begin = std::fmin(t_begin, t_end); c->t_end = std::fmax(t_begin, t_end);
    c->bvh.cx = bb.centre[0]; c->bvh.cy = bb.centre[1]; c->bvh.cz = bb.centre[2];
    c->bvh.centre_radius = bb.centre_radius;
    c->bvh.r_max2 = bb.r_max * bb.r_max * 1.000001f;
    c->bvh.inv_2rmin = bb.r_min > 0.0f ? 1.0f / (2.0f * bb.r_min) : INFINITY;
    c->bvh.abs_max = bb.abs_max;

    c->sc.geom = m.geom.as<f4>(); c->sc.vel = m.vel.as<f4>(); c->sc.mat = m.mat.as<DevMat>();
    c->sc.tex = m.tex.as<RtwTexture>(); c->sc.texels = m.texels.as<float>();
    c->scene_mem = std::move(m);
    c->sc.n = s->n_spheres; c->sc.moving = moving ? 1u : 0u;
    std::memcpy(c->bg, s->background, sizeof c->bg);
    c->has_textures = false;
    for (uint32_t i = 0; i < s->n_spheres; i++) if (s->spheres[i].tex >= 0) c->has_textures = true;
    // which textures the primitives read: noise on any of them selects the noise build (rtw_ctx_set_texture_noise)
    c->n_textures = s->n_textures;
    c->tex_used.assign(s->n_textures, 0);
    for (uint32_t i = 0; i < s->n_spheres; i++) if (s->spheres[i].tex >= 0) c->tex_used[s->spheres[i].tex] = 1;
    for (uint32_t i = 0; i < s->n_inst_spheres; i++) if (s->inst_spheres[i].tex >= 0) c->tex_used[s->inst_spheres[i].tex] = 1;
    for (uint32_t i = 0; i < s->n_quads; i++) if (s->quads[i].tex >= 0) c->tex_used[s->quads[i].tex] = 1;
    for (uint32_t i = 0; i < s->n_inst_quads; i++) if (s->inst_quads[i].tex >= 0) c->tex_used[s->inst_quads[i].tex] = 1;
    c->h_spheres.assign(s->spheres, s->spheres + s->n_spheres);
    c->h_quads.assign(s->quads, s->quads + s->n_quads);
    c->h_instances.assign(s->instances, s->instances + s->n_instances);
    for (uint32_t i = 0; i < s->n_instances; i++) if (s->instances[i].medium == RTW_MEDIUM_CONST_DENSITY) c->has_medium = true;
    scene_mixed(s, c->has_mixed, c->mixed_bad);
    c->has_scene = true;
    return RTW_OK;
}

// ---- lights (rtw.h "light-biased integrators") ----------------------------------------------------------------------------------------
// The argument checks shared by rtw_ctx_set_lights and rtw_light_mid, and the light's row {mid-point, object code}.
static int light_row_of(const RtwSphere *spheres, uint32_t n_spheres, const RtwQuad *quads, uint32_t n_quads, const RtwLight &l, float row[4]) {
    uint32_t code;
    if (l.kind == RTW_LIGHT_SPHERE) {
        if (l.index >= n_spheres || !spheres) return RTW_E_INVALID;
        light_mid_sphere(spheres[l.index].center, spheres[l.index].radius, row);
        code = l.index;
    } else if (l.kind == RTW_LIGHT_QUAD) {
        if (l.index >= n_quads || !quads || l.index >= LIGHT_HIT_QUAD) return RTW_E_INVALID;
        light_mid_quad(quads[l.index].origin, quads[l.index].u, quads[l.index].v, row);
        code = LIGHT_HIT_QUAD | l.index;
    } else return RTW_E_INVALID;
    std::memcpy(&row[3], &code, sizeof code);
    return RTW_OK;
}

int rtw_light_mid(const RtwScene *scene, const RtwLight *light, float mid[3]) {
    if (!scene || !light || !mid) return RTW_E_INVALID;
    float row[4];
    const int rc = light_row_of(scene->spheres, scene->n_spheres, scene->quads, scene->n_quads, *light, row);
    if (rc != RTW_OK) return rc;
    mid[0] = row[0]; mid[1] = row[1]; mid[2] = row[2];
    return RTW_OK;
}

float rtw_material_pdf(const float mat3[3], const float p[3], const float n[3], const float dir_in[3], float time_in,
                       const float ray_o[3], const float ray_d[3], float ray_time) {
    if (!mat3 || !p || !n || !dir_in || !ray_o || !ray_d) return NAN;
    return light_material_pdf(mat3[0], mat3[1], mat3[2], lmk(p[0], p[1], p[2]), lmk(n[0], n[1], n[2]), lmk(dir_in[0], dir_in[1], dir_in[2]), time_in,
                              lmk(ray_o[0], ray_o[1], ray_o[2]), lmk(ray_d[0], ray_d[1], ray_d[2]), ray_time);
}

int rtw_light_term(uint32_t integrator, float pdf, const float e[3], float t, const float dir[3], float biased_weight, float S[3], float *count) {
    if (!e || !dir || !S || !count) return RTW_E_INVALID;
    if (integrator != RTW_INTEGRATOR_LIGHT_CAST && integrator != RTW_INTEGRATOR_LIGHT_BIASED) return RTW_E_INVALID;
    lv3 s = lmk(S[0], S[1], S[2]);
    const bool added = light_add(integrator == RTW_INTEGRATOR_LIGHT_BIASED, pdf, lmk(e[0], e[1], e[2]), t, lmk(dir[0], dir[1], dir[2]), biased_weight, s, *count);
    S[0] = s.x; S[1] = s.y; S[2] = s.z;
    return added ? 1 : 0;
}

// The checks of a light list against a scene's top-level spheres and quads, and its rows: shared by rtw_lights_validate (host only) and
// rtw_ctx_set_lights.  rows may be null.
static int lights_check(const RtwSphere *spheres, uint32_t n_spheres, const RtwQuad *quads, uint32_t n_quads, const RtwLight *lights, uint32_t n,
                        float (*rows)[4]) {
    if ((n && !lights) || (!n && lights) || n > RTW_MAX_LIGHTS) return RTW_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        float row[4];
        const int rc = light_row_of(spheres, n_spheres, quads, n_quads, lights[i], row);
        if (rc != RTW_OK) return rc;
        if (rows) std::memcpy(rows[i], row, sizeof row);
    }
    return RTW_OK;
}

int rtw_lights_validate(const RtwScene *scene, const RtwLight *lights, uint32_t n) {
    if (!scene) return RTW_E_INVALID;
    return lights_check(scene->spheres, scene->n_spheres, scene->quads, scene->n_quads, lights, n, nullptr);
}

int rtw_ctx_set_lights(rtw_ctx *c, const RtwLight *lights, uint32_t n, float biased_weight) {
    if (!c) return RTW_E_INVALID;
    if (!c->has_scene) return RTW_E_NO_SCENE;
    if (c->pend.active) return RTW_E_INVALID;
    DevLights d{};
    const int rc = lights_check(c->h_spheres.data(), (uint32_t)c->h_spheres.size(), c->h_quads.data(), (uint32_t)c->h_quads.size(), lights, n, d.row);
    if (rc != RTW_OK) return rc;
    d.n = n; d.weight = biased_weight;
    c->lights = d;
    c->light_rows.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        const RtwLight &l = lights[i];
        c->light_rows[i] = l.kind == RTW_LIGHT_SPHERE ? direct_row_sphere(c->h_spheres[l.index].center, c->h_spheres[l.index].radius)
                                                      : direct_row_quad(c->h_quads[l.index].origin, c->h_quads[l.index].u, c->h_quads[l.index].v);
    }
    return RTW_OK;
}

// ---- Rust2's instance rotations (rtw.h "quaternion-rotated instances") ------------------------------------------------------------------
// The checks of a rotation list against a scene's instances, and the rows the kernels read (the normalised quaternions, formed with the
// operations of Quaternion::rotate): shared by rtw_instance_rotations_validate (host only) and rtw_ctx_set_instance_rotations.  rows may be null.
static int quats_check(const RtwInstance *inst, uint32_t n_inst, const float (*qs)[4], uint32_t n, f4 *rows) {
    if (!qs || n != n_inst || (n && !inst)) return RTW_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        const quat q = qmk(qs[i][0], qs[i][1], qs[i][2], qs[i][3]);
        if (!std::isfinite(q.w) || !std::isfinite(q.x) || !std::isfinite(q.y) || !std::isfinite(q.z)) return RTW_E_INVALID;
        const float l = quat_len(q);
        if (!(l > 0.0f) || !std::isfinite(l)) return RTW_E_INVALID;
        if (inst[i].rotation[0] != 0.0f || inst[i].rotation[1] != 0.0f || inst[i].rotation[2] != 0.0f) return RTW_E_INVALID;   // one rotation per instance
        if (inst[i].medium != RTW_MEDIUM_SURFACE) return RTW_E_INVALID;       // constant density is Rust/'s: the reference defines no mix of the two
        const quat qn = quat_normalised(q);
        if (rows) { f4 r; r.x = qn.w; r.y = qn.x; r.z = qn.y; r.w = qn.z; rows[i] = r; }
    }
    return RTW_OK;
}

int rtw_instance_rotations_validate(const RtwScene *scene, const float (*qs)[4], uint32_t n) {
    if (!scene) return RTW_E_INVALID;
    if (!qs && n == 0) return RTW_OK;
    return quats_check(scene->instances, scene->n_instances, qs, n, nullptr);
}

int rtw_ctx_set_instance_rotations(rtw_ctx *c, const float (*qs)[4], uint32_t n) {
    if (!c) return RTW_E_INVALID;
    if (!c->has_scene) return RTW_E_NO_SCENE;
    if (c->pend.active) return RTW_E_INVALID;
    std::vector<f4> rows;
    if (qs || n) {
        if (!qs || n != c->h_instances.size()) return RTW_E_INVALID;            // (before anything is sized by the caller's n)
        try { rows.resize(n); } catch (const std::bad_alloc &) { return RTW_E_NOMEM; }
        const int rc = quats_check(c->h_instances.data(), (uint32_t)c->h_instances.size(), qs, n, rows.data());
        if (rc != RTW_OK) return rc;
    }
    HIP_TRY(hipSetDevice(c->device));
    free_quats(c);
    if (!n) return RTW_OK;                                         // NULL / 0, or a scene without instances: nothing to rotate
    QuatMem m;
    if (const int rc = upload(m.rows, rows)) return rc;
    c->inst_quats = m.rows.as<f4>();
    c->quat_mem = std::move(m);
    return RTW_OK;
}

// What a render answers while instance rotations are set: the quaternion build serves Rust2's three integrators, and nothing is built for
// texture noise or triangles next to it.
static int quats_render_check(bool rotations, uint32_t integrator, bool noise, bool tris) {
    if (!rotations) return RTW_OK;
    if (integrator != RTW_INTEGRATOR_RUST2 && integrator != RTW_INTEGRATOR_LIGHT_CAST && integrator != RTW_INTEGRATOR_LIGHT_BIASED) return RTW_E_INVALID;
    if (noise || tris) return RTW_E_INVALID;
    return RTW_OK;
}

int rtw_quat_rotate(const float q[4], const float v[3], float out[3]) {
    if (!q || !v || !out) return RTW_E_INVALID;
    float x, y, z;
    quat_rotate(qmk(q[0], q[1], q[2], q[3]), v[0], v[1], v[2], x, y, z);
    out[0] = x; out[1] = y; out[2] = z;
    return RTW_OK;
}
int rtw_quat_mul(const float a[4], const float b[4], float out[4]) {
    if (!a || !b || !out) return RTW_E_INVALID;
    const quat r = quat_hamilton(qmk(a[0], a[1], a[2], a[3]), qmk(b[0], b[1], b[2], b[3]));
    out[0] = r.w; out[1] = r.x; out[2] = r.y; out[3] = r.z;
    return RTW_OK;
}
int rtw_quat_from_axis(float angle, const float axis[3], float out[4]) {
    if (!axis || !out) return RTW_E_INVALID;
    const quat r = quat_from_axis(angle, axis[0], axis[1], axis[2]);
    out[0] = r.w; out[1] = r.x; out[2] = r.y; out[3] = r.z;
    return RTW_OK;
}
int rtw_quat_from_euler(const float euler[3], float out[4]) {
    if (!euler || !out) return RTW_E_INVALID;
    const quat r = quat_from_euler(euler[0], euler[1], euler[2]);
    out[0] = r.w; out[1] = r.x; out[2] = r.y; out[3] = r.z;
    return RTW_OK;
}

int rtw_ctx_set_texture_noise(rtw_ctx *c, const RtwPerlin *tables, uint32_t n_tables, const RtwTextureNoise *per_texture, uint32_t n_textures) {
    if (!c) return RTW_E_INVALID;
    if (!c->has_scene) return RTW_E_NO_SCENE;
    if (c->pend.active) return RTW_E_INVALID;
    if (!per_texture) {                                            // NULL / 0: no noise
        if (n_textures != 0) return RTW_E_INVALID;
        HIP_TRY(hipSetDevice(c->device));
        free_noise(c);
        return RTW_OK;
    }
    if (n_textures != c->n_textures || (n_tables && !tables)) return RTW_E_INVALID;
    if (c->tris.n) return RTW_E_UNSUPPORTED;                       // texture noise on triangles: not implemented
    bool active = false;
    for (uint32_t i = 0; i < n_textures; i++) {
        const int32_t k = per_texture[i].perlin;
        if (k < -1 || (k >= 0 && (uint32_t)k >= n_tables)) return RTW_E_INVALID;
        if (k >= 0 && c->tex_used[i]) active = true;
    }
    HIP_TRY(hipSetDevice(c->device));
    free_noise(c);
    if (!active) return RTW_OK;                                    // no texture a primitive reads has noise: the image is the noise-free one
    std::vector<RtwPerlin> tb(tables, tables + n_tables);
    std::vector<RtwTextureNoise> tn(per_texture, per_texture + n_textures);
    NoiseMem m;
    int rc;
    if ((rc = upload(m.perlin, tb)) || (rc = upload(m.tex_noise, tn))) return rc;
    c->noise.tables = m.perlin.as<RtwPerlin>();
    c->noise.tex = m.tex_noise.as<RtwTextureNoise>();
    c->noise_mem = std::move(m);
    c->noise_active = true;
    return RTW_OK;
}

int rtw_ctx_set_triangles(rtw_ctx *c, const RtwTriangle *tris, uint32_t n) {
    if (!c) return RTW_E_INVALID;
    if (!c->has_scene) return RTW_E_NO_SCENE;
    if (c->pend.active || (n && !tris) || (!n && tris)) return RTW_E_INVALID;
    for (uint32_t i = 0; i < n; i++) if (tris[i].tex < -1 || tris[i].tex >= (int32_t)c->n_textures) return RTW_E_INVALID;
    if (n && c->noise_active) return RTW_E_UNSUPPORTED;
    HIP_TRY(hipSetDevice(c->device));
    free_tris(c);
    if (!n) return RTW_OK;
    std::vector<DevTri> list;
    TriBuild b;
    try { list.resize(n); } catch (const std::bad_alloc &) { return RTW_E_NOMEM; }
    tri_prepare(tris, n, list.data());
    if (!tri_build(list.data(), n, b)) return RTW_E_NOMEM;
    std::vector<DevTri> leaf(b.leaf, b.leaf + n);
    std::vector<TriNode> nodes(b.nodes, b.nodes + b.n_nodes);
    RefitSchedule sched;
    if (!tri_refit_schedule(b.nodes, b.n_nodes, sched)) return RTW_E_NOMEM;
    TriMem m;
    int rc;
    if ((rc = upload(m.list, list)) || (rc = upload(m.leaf, leaf)) || (rc = upload(m.nodes, nodes))) return rc;
    // everything a refit needs, now: rtw_ctx_refit_triangles reserves nothing
    if ((rc = upload(m.order, sched.order))) return rc;
    HIP_TRY(m.ouv.reserve(REFIT_OUV_BYTES * (size_t)n));
    HIP_TRY(m.bad.reserve(sizeof(uint32_t)));
    HIP_TRY(c->scr.h_refit.reserve(REFIT_READBACK_BYTES));
    c->refit_first = std::move(sched.first);
    c->tris.list = m.list.as<DevTri>(); c->tris.leaf = m.leaf.as<DevTri>();
    c->tris.n = n; c->tris.n_nodes = b.n_nodes;
    c->tri_tree = !b.list_walk;
    c->tri_root = b.nodes[0];
    c->tri_mem = std::move(m);
    for (uint32_t i = 0; i < n; i++) if (tris[i].tex >= 0) c->tri_textured = true;
    return RTW_OK;
}

// The triangles move, the tree's topology stays (rtw.h "refit"; device code: rtw_refit.hip).  On the context's stream, behind the caller's
// producers of `ouv`; one synchronise at the end for the count of refused triangles and the new root.
int rtw_ctx_refit_triangles(rtw_ctx *c, const float *ouv, uint32_t n, uint32_t *list_walk_out) {
    if (!c) return RTW_E_INVALID;
    if (!c->tris.n) return RTW_E_NO_SCENE;
    if (!ouv || n != c->tris.n || c->pend.active || c->mesh_rows) return RTW_E_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    TriMem &m = c->tri_mem;
    unsigned char *back = c->scr.h_refit.as<unsigned char>();
    hipError_t e = hipSuccess;
    const float *src = ouv;
    if (!on_device(ouv, c->device)) {
        e = hipMemcpyAsync(m.ouv.ptr, ouv, REFIT_OUV_BYTES * (size_t)n, hipMemcpyDefault, c->stream);
        src = m.ouv.as<const float>();
    }
    if (e == hipSuccess) e = hipMemsetAsync(m.bad.ptr, 0, sizeof(uint32_t), c->stream);
    if (e == hipSuccess) {
        launch_tri_refit(m.nodes.as<TriNode>(), m.leaf.as<DevTri>(), m.list.as<DevTri>(), src, m.order.as<const uint32_t>(), c->refit_first.data(),
                         (uint32_t)c->refit_first.size() - 1u, m.bad.as<uint32_t>(), c->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(back, m.bad.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(back + 32, m.nodes.ptr, sizeof(TriNode), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    // a refit that stopped half-way: the records may be partly moved, so the tree is not walked (the list answers from whatever the records
    // hold) and tri_root is marked stale -- rtw_ctx_set_mesh_instances would form its world boxes from it
    if (const int rc = call_status(c, e)) { c->tri_tree = false; c->tri_root_stale = true; return rc; }
    uint32_t bad;
    std::memcpy(&bad, back, sizeof bad);
    std::memcpy(&c->tri_root, back + 32, sizeof(TriNode));
    c->tri_tree = bad == 0;
    c->tri_root_stale = false;
    if (list_walk_out) *list_walk_out = bad ? 1u : 0u;
    return RTW_OK;
}

int rtw_ctx_triangle_bvh_dump(rtw_ctx *c, RtwTriNode *nodes_out, uint32_t node_cap, uint32_t *n_nodes) {
    static_assert(sizeof(RtwTriNode) == sizeof(TriNode), "the public node is the device's");
    if (!c) return RTW_E_INVALID;
    if (!c->tris.n) return RTW_E_NO_SCENE;
    if (c->pend.active) return RTW_E_INVALID;
    if (n_nodes) *n_nodes = c->tris.n_nodes;
    if (!nodes_out) return RTW_OK;
    if (node_cap < c->tris.n_nodes) return RTW_E_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    hipError_t e = hipMemcpyAsync(nodes_out, c->tri_mem.nodes.ptr, c->tris.n_nodes * sizeof(TriNode), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return call_status(c, e);
}

// ---- mesh placements (rtw.h "mesh placements"; device code: rtw_mesh.h) -----------------------------------------------------------------
int rtw_ctx_set_mesh_instances(rtw_ctx *c, const RtwMeshInstance *p, uint32_t n) {
    if (!c) return RTW_E_INVALID;
    if (!c->tris.n) return RTW_E_NO_SCENE;
    if (c->pend.active || (n && !p) || (!n && p) || n > RTW_MAX_MESH_INSTANCES) return RTW_E_INVALID;
    std::vector<f4> rows;
    if (n) {
        if (c->tri_textured || c->tri_root_stale) return RTW_E_INVALID;
        try { rows.resize(2 * (size_t)n); } catch (const std::bad_alloc &) { return RTW_E_NOMEM; }
        if (!mesh_rows(p, n, rows.data())) return RTW_E_INVALID;
    }
    HIP_TRY(hipSetDevice(c->device));
    free_mesh(c);
    if (!n) return RTW_OK;
    // the top-level tree and its height schedule, always -- beyond reach too: a later move may bring the placements back (whether a render
    // walks it: mesh_top_view; n == 1: one leaf that only the move's placement pass reads)
    MeshTopBuild top;
    std::vector<unsigned char> packed;
    RefitSchedule sched;
    if (!mesh_top_build(c->tri_root, rows.data(), n, top)) return RTW_E_NOMEM;
    try { packed = top.packed(); } catch (const std::bad_alloc &) { return RTW_E_NOMEM; }
    if (!tri_refit_schedule(top.nodes.data(), (uint32_t)top.nodes.size(), sched)) return RTW_E_NOMEM;
    MeshMem m;
    int rc;
    if ((rc = upload(m.rows, rows)) || (rc = upload(m.top, packed))) return rc;
    // everything a move needs, now: rtw_ctx_move_mesh_instances reserves nothing
    if ((rc = upload(m.order, sched.order)) || (rc = upload(m.first, sched.first))) return rc;
    HIP_TRY(m.poses.reserve(MOVE_POSE_BYTES * (size_t)n));
    HIP_TRY(m.counts.reserve(2 * sizeof(uint32_t)));
    c->mesh_rows = m.rows.as<f4>(); c->n_mesh = n;
    c->n_top_nodes = (uint32_t)top.nodes.size();
    if (n >= 2) { c->mesh_top = m.top.as<TriNode>(); c->n_mesh_top = c->n_top_nodes; }
    c->mesh_top_ok = !top.list_walk;
    c->move_first = std::move(sched.first);
    c->mesh_mem = std::move(m);
    return RTW_OK;
}

// The placements move, the mesh may move with them, both trees keep their topology (rtw.h "moving placements"; device code: rtw_mesh_move.hip).
// On the context's stream, behind the caller's producers of `poses` and `ouv`: the triangle refit (when ouv is given), the placement pass
// -- which reads the mesh's root from the device's node 0, so no host round trip stands between the two --, the climb; one synchronise at
// the end for the counts and the mesh's root.
static bool mesh_climb_choice(const rtw_ctx *c) {
    return c->opt_mesh_climb == 0 ? mesh_climb_one_group(c->n_top_nodes) : c->opt_mesh_climb == 2;
}
int rtw_ctx_move_mesh_instances(rtw_ctx *c, const float *poses, uint32_t n, const float *ouv, uint32_t n_tris, uint32_t *list_walk_out) {
    if (!c) return RTW_E_INVALID;
    if (!c->mesh_rows) return RTW_E_NO_SCENE;
    if ((!poses && !ouv) || (poses && n != c->n_mesh) || (ouv && n_tris != c->tris.n) || c->pend.active || (!ouv && c->tri_root_stale)) return RTW_E_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    TriMem &t = c->tri_mem;
    MeshMem &m = c->mesh_mem;
    unsigned char *back = c->scr.h_refit.as<unsigned char>();
    hipError_t e = hipSuccess;
    const float *src_ouv = ouv, *src_poses = poses;
    if (ouv && !on_device(ouv, c->device)) {
        e = hipMemcpyAsync(t.ouv.ptr, ouv, REFIT_OUV_BYTES * (size_t)n_tris, hipMemcpyDefault, c->stream);
        src_ouv = t.ouv.as<const float>();
    }
    if (e == hipSuccess && poses && !on_device(poses, c->device)) {
        e = hipMemcpyAsync(m.poses.ptr, poses, MOVE_POSE_BYTES * (size_t)n, hipMemcpyDefault, c->stream);
        src_poses = m.poses.as<const float>();
    }
    if (e == hipSuccess) e = hipMemsetAsync(t.bad.ptr, 0, sizeof(uint32_t), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(m.counts.ptr, 0, 2 * sizeof(uint32_t), c->stream);
    if (e == hipSuccess) {
        if (ouv) launch_tri_refit(t.nodes.as<TriNode>(), t.leaf.as<DevTri>(), t.list.as<DevTri>(), src_ouv, t.order.as<const uint32_t>(), c->refit_first.data(),
                                  (uint32_t)c->refit_first.size() - 1u, t.bad.as<uint32_t>(), c->stream);
        launch_mesh_move(m.top.as<TriNode>(), (const uint32_t *)(m.top.as<TriNode>() + c->n_top_nodes), m.rows.as<f4>(), src_poses, t.nodes.as<const TriNode>(),
                         m.order.as<const uint32_t>(), c->move_first.data(), m.first.as<const uint32_t>(), (uint32_t)c->move_first.size() - 1u,
                         mesh_climb_choice(c), m.counts.as<uint32_t>(), c->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(back, t.bad.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(back + 8, m.counts.ptr, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(back + 32, t.nodes.ptr, sizeof(TriNode), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    // a move that stopped half-way: rows and boxes may be partly moved, so neither tree is walked (the lists answer from whatever the records
    // hold) and tri_root is marked stale, as after a refit that stopped
    if (const int rc = call_status(c, e)) { c->tri_tree = false; c->tri_root_stale = true; c->mesh_top_ok = false; return rc; }
    uint32_t bad, counts[2];
    std::memcpy(&bad, back, sizeof bad);
    std::memcpy(counts, back + 8, sizeof counts);
    std::memcpy(&c->tri_root, back + 32, sizeof(TriNode));
    if (ouv) { c->tri_tree = bad == 0; c->tri_root_stale = false; }
    c->mesh_top_ok = counts[1] == 0;
    if (list_walk_out) *list_walk_out = (c->tri_tree ? 0u : 1u) | (counts[1] ? 2u : 0u);
    return counts[0] ? RTW_E_INVALID : RTW_OK;
}

int rtw_ctx_mesh_top_dump(rtw_ctx *c, RtwTriNode *nodes_out, uint32_t node_cap, uint32_t *n_nodes, float *rows_out) {
    if (!c) return RTW_E_INVALID;
    if (!c->mesh_rows) return RTW_E_NO_SCENE;
    if (c->pend.active) return RTW_E_INVALID;
    if (n_nodes) *n_nodes = c->n_top_nodes;
    if (!nodes_out && !rows_out) return RTW_OK;
    if (nodes_out && node_cap < c->n_top_nodes) return RTW_E_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    hipError_t e = hipSuccess;
    if (nodes_out) e = hipMemcpyAsync(nodes_out, c->mesh_mem.top.ptr, c->n_top_nodes * sizeof(TriNode), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && rows_out) e = hipMemcpyAsync(rows_out, c->mesh_mem.rows.ptr, 2 * (size_t)c->n_mesh * sizeof(f4), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return call_status(c, e);
}

// What a render answers while placements are set: the placement build serves RTW_INTEGRATOR_RUST2; nothing is built for a MixedMaterial
// object or instance rotations next to it.
static int mesh_render_check(bool placements, uint32_t integrator, bool mixed_active, bool rotations) {
    if (!placements) return RTW_OK;
    if (integrator != RTW_INTEGRATOR_RUST2 || mixed_active || rotations) return RTW_E_INVALID;
    return RTW_OK;
}

int rtw_ctx_triangle_hits(rtw_ctx *c, const float *rays, uint32_t n_rays, float mint, float maxt, uint32_t accel,
                          float *t_out, int32_t *idx_out, RtwStats *stats) {
    if (!c || !rays || !t_out || !idx_out || n_rays == 0 || accel > RTW_ACCEL_BVH) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    if (!c->tris.n) return RTW_E_NO_SCENE;
    HIP_TRY(hipSetDevice(c->device));
    const DevTris T = tri_view(c, accel, mint, maxt);
    const size_t t_bytes = sizeof(float) * (size_t)n_rays, i_bytes = sizeof(int32_t) * (size_t)n_rays;
    Staging st(c, true);
    unsigned long long cnt[2] = { 0, 0 };
    const float *d_r = st.in(rays, 6 * t_bytes);
    float *d_t = st.out(t_out, t_bytes);
    int32_t *d_i = st.out(idx_out, i_bytes);
    unsigned long long *d_c = st.out(cnt, sizeof cnt);
    if (st.e == hipSuccess) st.e = hipMemsetAsync(d_c, 0, sizeof cnt, c->stream);
    if (st.e == hipSuccess) {
        launch_tri_hits(T, d_r, n_rays, mint, maxt, d_t, d_i, d_c, c->stream);
        st.e = hipGetLastError();
    }
    if (const int rc = st.finish()) return rc;
    if (stats) { std::memset(stats, 0, sizeof *stats); stats->quad_tests = cnt[0]; stats->node_tests = cnt[1]; }
    return RTW_OK;
}

int rtw_ctx_mesh_instance_hits(rtw_ctx *c, const float *rays, uint32_t n_rays, float mint, float maxt, uint32_t accel,
                               float *t_out, int32_t *placement_out, int32_t *tri_out, float *normal_out, RtwStats *stats) {
    if (!c || !rays || !t_out || !placement_out || !tri_out || n_rays == 0 || accel > RTW_ACCEL_BVH) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    if (!c->mesh_rows) return RTW_E_NO_SCENE;
    HIP_TRY(hipSetDevice(c->device));
    const DevTris T = tri_view(c, accel, mint, maxt);
    const size_t t_bytes = sizeof(float) * (size_t)n_rays, i_bytes = sizeof(int32_t) * (size_t)n_rays;
    Staging st(c, true);
    unsigned long long cnt[2] = { 0, 0 };
    const float *d_r = st.in(rays, 6 * t_bytes);
    float *d_t = st.out(t_out, t_bytes);
    int32_t *d_p = st.out(placement_out, i_bytes);
    int32_t *d_i = st.out(tri_out, i_bytes);
    float *d_n = normal_out ? st.out(normal_out, 3 * t_bytes) : nullptr;
    unsigned long long *d_c = st.out(cnt, sizeof cnt);
    if (st.e == hipSuccess) st.e = hipMemsetAsync(d_c, 0, sizeof cnt, c->stream);
    if (st.e == hipSuccess) {
        launch_mesh_hits(T, c->mesh_rows, c->n_mesh, mesh_top_view(c, T), c->n_mesh_top, d_r, n_rays, mint, maxt, d_t, d_p, d_i, d_n, d_c, c->stream);
        st.e = hipGetLastError();
    }
    if (const int rc = st.finish()) return rc;
    if (stats) { std::memset(stats, 0, sizeof *stats); stats->quad_tests = cnt[0]; stats->node_tests = cnt[1]; }
    return RTW_OK;
}

// ---- scene ray queries (rtw.h "scene ray queries"; kernel: rtw_query.hip) ------------------------------------------------------------
// What the surface calls ask of the pass on top of a query (rtw.h "surface buffers"): the winner's record under `integrator`, and the rule of
// the camera's rays.
struct SurfaceAsk {
    float *albedo, *emitted, *material;
    uint32_t integrator, ray_rule;
    float off_x, off_y;
    int32_t *tri; float *bary;           // (the _tri calls; either may be null)
};

// All four calls: cam != null builds the rays of a width x height map in the kernel, else `rays` [n][6] are read.  sf != null: the surface
// builds of the kernel.
static int scene_query(rtw_ctx *c, const RtwCamera *cam, uint32_t width, uint32_t height, const float *rays, uint32_t n, float time, float mint,
                       float maxt, uint32_t accel, float miss_t, float *t_out, int32_t *idx_out, float *normal_out, RtwStats *stats,
                       const SurfaceAsk *sf = nullptr) {
    if (c->pend.active) return RTW_E_INVALID;
    if (!c->has_scene) return RTW_E_NO_SCENE;
    if (sf && c->noise_active) return RTW_E_INVALID;               // not built: the record of a texture with noise
    HIP_TRY(hipSetDevice(c->device));
    const bool tree = query_uses_tree(c, accel, time, mint, maxt);

    QueryArgs q;
    scene_views(c, n, time, mint, maxt, accel, q);
    if (cam) { q.cam = *cam; q.width = width; q.height = height; }
    q.miss_t = miss_t;

    const size_t t_bytes = sizeof(float) * (size_t)n;
    Staging st(c);
    if (rays) q.rays = st.in(rays, 6 * t_bytes);
    q.t_out = st.out(t_out, t_bytes);
    if (idx_out) q.idx_out = st.out(idx_out, sizeof(int32_t) * (size_t)n);
    if (normal_out) q.normal_out = st.out(normal_out, 3 * t_bytes);
    if (sf) {
        q.albedo_out = st.out(sf->albedo, 3 * t_bytes);
        if (sf->emitted) q.emitted_out = st.out(sf->emitted, 3 * t_bytes);
        if (sf->material) q.material_out = st.out(sf->material, 3 * t_bytes);
        q.rust2 = sf->integrator == RTW_INTEGRATOR_RUST2 || sf->integrator == RTW_INTEGRATOR_LIGHT_CAST || sf->integrator == RTW_INTEGRATOR_LIGHT_BIASED;
        q.ray_rule = sf->ray_rule; q.off_x = sf->off_x; q.off_y = sf->off_y;
        if (sf->tri) q.tri_out = st.out(sf->tri, sizeof(int32_t) * (size_t)n);
        if (sf->bary) q.bary_out = st.out(sf->bary, 2 * t_bytes);
        if (st.e == hipSuccess && !q.albedo_out) st.e = hipErrorInvalidValue;      // (albedo_out selects the build)
    }
    return counted_pass(c, st, 0, n, stats, [&] { launch_scene_hits(q, cam != nullptr, tree, c->stream); });
}

int rtw_ctx_scene_hits(rtw_ctx *c, const float *rays, uint32_t n_rays, float time, float mint, float maxt, uint32_t accel,
                       float *t_out, int32_t *idx_out, float *normal_out, RtwStats *stats) {
    if (!c || !rays || !t_out || !idx_out || n_rays == 0 || accel > RTW_ACCEL_BVH) return RTW_E_INVALID;
    return scene_query(c, nullptr, 0, 0, rays, n_rays, time, mint, maxt, accel, std::numeric_limits<float>::infinity(), t_out, idx_out, normal_out, stats);
}

int rtw_ctx_depth_map(rtw_ctx *c, const RtwCamera *cam, uint32_t width, uint32_t height, float time, float mint, float maxt, uint32_t accel,
                      float *depth_out, int32_t *idx_out, float *normal_out, RtwStats *stats) {
    if (!c || !cam || !depth_out || width == 0 || height == 0 || accel > RTW_ACCEL_BVH) return RTW_E_INVALID;
    if ((uint64_t)width * height > 0xFFFFFFFFull) return RTW_E_INVALID;
    return scene_query(c, cam, width, height, nullptr, width * height, time, mint, maxt, accel, host_mul(maxt, 1.6f), depth_out, idx_out, normal_out, stats);
}

// The surface buffers (rtw.h "surface buffers"): the same pass, the winner's hit record written beside t, idx and normal
int rtw_ctx_scene_surface_tri(rtw_ctx *c, const float *rays, uint32_t n_rays, float time, float mint, float maxt, uint32_t accel, uint32_t integrator,
                              float *t_out, int32_t *idx_out, float *normal_out, float *albedo_out, float *emitted_out, float *material_out,
                              int32_t *tri_out, float *bary_out, RtwStats *stats) {
    if (!c || !rays || !t_out || !idx_out || n_rays == 0 || accel > RTW_ACCEL_BVH) return RTW_E_INVALID;
    if (!albedo_out || integrator > RTW_INTEGRATOR_LIGHT_BIASED) return RTW_E_INVALID;
    const SurfaceAsk sf = { albedo_out, emitted_out, material_out, integrator, RTW_RAYS_DEPTH_MAP, 0.0f, 0.0f, tri_out, bary_out };
    return scene_query(c, nullptr, 0, 0, rays, n_rays, time, mint, maxt, accel, std::numeric_limits<float>::infinity(), t_out, idx_out, normal_out, stats,
                       &sf);
}
int rtw_ctx_scene_surface(rtw_ctx *c, const float *rays, uint32_t n_rays, float time, float mint, float maxt, uint32_t accel, uint32_t integrator,
                          float *t_out, int32_t *idx_out, float *normal_out, float *albedo_out, float *emitted_out, float *material_out,
                          RtwStats *stats) {
    return rtw_ctx_scene_surface_tri(c, rays, n_rays, time, mint, maxt, accel, integrator, t_out, idx_out, normal_out, albedo_out, emitted_out,
                                     material_out, nullptr, nullptr, stats);
}

int rtw_ctx_surface_map_tri(rtw_ctx *c, const RtwCamera *cam, uint32_t width, uint32_t height, uint32_t ray_rule, const float *offset, float time,
                            float mint, float maxt, uint32_t accel, uint32_t integrator, float *depth_out, int32_t *idx_out, float *normal_out,
                            float *albedo_out, float *emitted_out, float *material_out, int32_t *tri_out, float *bary_out, RtwStats *stats) {
    if (!c || !cam || !depth_out || width == 0 || height == 0 || accel > RTW_ACCEL_BVH) return RTW_E_INVALID;
    if ((uint64_t)width * height > 0xFFFFFFFFull) return RTW_E_INVALID;
    if (!albedo_out || integrator > RTW_INTEGRATOR_LIGHT_BIASED || ray_rule > RTW_RAYS_PIXEL) return RTW_E_INVALID;
    const SurfaceAsk sf = { albedo_out, emitted_out, material_out, integrator, ray_rule, offset ? offset[0] : 0.0f, offset ? offset[1] : 0.0f,
                            tri_out, bary_out };
    return scene_query(c, cam, width, height, nullptr, width * height, time, mint, maxt, accel, host_mul(maxt, 1.6f), depth_out, idx_out, normal_out,
                       stats, &sf);
}
int rtw_ctx_surface_map(rtw_ctx *c, const RtwCamera *cam, uint32_t width, uint32_t height, uint32_t ray_rule, const float *offset, float time,
                        float mint, float maxt, uint32_t accel, uint32_t integrator, float *depth_out, int32_t *idx_out, float *normal_out,
                        float *albedo_out, float *emitted_out, float *material_out, RtwStats *stats) {
    return rtw_ctx_surface_map_tri(c, cam, width, height, ray_rule, offset, time, mint, maxt, accel, integrator, depth_out, idx_out, normal_out,
                                   albedo_out, emitted_out, material_out, nullptr, nullptr, stats);
}

// The any-hit pass (rtw.h "occlusion queries"; kernel: rtw_occluded.hip): scene_query's conditions, views, staging and stream order
int rtw_ctx_scene_occluded(rtw_ctx *c, const float *rays, uint32_t n, float time, float mint, float maxt, uint32_t accel, uint8_t *occluded_out,
                           RtwStats *stats) {
    if (!c || !rays || !occluded_out || n == 0 || accel > RTW_ACCEL_BVH) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    if (!c->has_scene) return RTW_E_NO_SCENE;
    HIP_TRY(hipSetDevice(c->device));
    const bool tree = query_uses_tree(c, accel, time, mint, maxt);

    OccludedArgs q;
    scene_views(c, n, time, mint, maxt, accel, q);
    Staging st(c);
    q.rays = st.in(rays, 6 * sizeof(float) * (size_t)n);
    q.out = st.out(occluded_out, n);
    return counted_pass(c, st, 0, n, stats, [&] { launch_scene_occluded(q, tree, c->stream); });
}

// ---- ambient occlusion (rtw.h "ambient occlusion"; the rule: rtw_ao.h) ------------------------------------------------------------------
int rtw_ctx_ambient_occlusion(rtw_ctx *c, const float *points, const float *normals, uint32_t n, uint32_t samples, uint32_t seed, float time,
                              float mint, float maxt, uint32_t accel, float *ao_out, RtwStats *stats) {
    if (!c || !points || !normals || !ao_out || n == 0 || !ao_samples_ok(samples) || accel > RTW_ACCEL_BVH) return RTW_E_INVALID;
    if ((uint64_t)n * samples > 0xFFFFFFFFull) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    if (!c->has_scene) return RTW_E_NO_SCENE;
    HIP_TRY(hipSetDevice(c->device));
    const bool tree = query_uses_tree(c, accel, time, mint, maxt);

    AoArgs a;
    fused_args(c, n, samples, seed, time, mint, maxt, accel, a);

    const size_t v_bytes = 3 * sizeof(float) * (size_t)n;
    Staging st(c);
    a.points = st.in(points, v_bytes);
    a.normals = st.in(normals, v_bytes);
    a.ao_out = st.out(ao_out, sizeof(float) * (size_t)n);
    return counted_pass(c, st, samples, 0, stats, [&] { launch_ambient_occlusion(a, false, tree, c->stream); });
}

// depth_pass, then the AO kernel's camera form over its outputs
int rtw_ctx_ao_map(rtw_ctx *c, const RtwCamera *cam, uint32_t width, uint32_t height, float time, float mint, float maxt, uint32_t samples,
                   uint32_t seed, float ao_mint, float ao_maxt, uint32_t accel, float *ao_out, float *depth_out, int32_t *idx_out,
                   float *normal_out, RtwStats *stats) {
    if (!c || !cam || !ao_out || width == 0 || height == 0 || !ao_samples_ok(samples) || accel > RTW_ACCEL_BVH) return RTW_E_INVALID;
    if ((uint64_t)width * height * samples > 0xFFFFFFFFull) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    if (!c->has_scene) return RTW_E_NO_SCENE;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t n = width * height;
    const bool tree = query_uses_tree(c, accel, time, mint, maxt), ao_tree = query_uses_tree(c, accel, time, ao_mint, ao_maxt);

    AoArgs a;
    fused_args(c, n, samples, seed, time, ao_mint, ao_maxt, accel, a);

    Staging st(c);
    a.ao_out = st.out(ao_out, sizeof(float) * (size_t)n);
    const QueryArgs q = depth_pass(c, st, cam, width, height, time, mint, maxt, accel, depth_out, idx_out, normal_out, a);
    return counted_pass(c, st, samples, n, stats, [&] { launch_scene_hits(q, true, tree, c->stream); },
                        [&] { launch_ambient_occlusion(a, true, ao_tree, c->stream); });
}

// ---- direct lighting (rtw.h "direct lighting"; the rule: rtw_direct.h) --------------------------------------------------------------------
// The statuses both calls share once their own arguments are in order; n: the points
static int direct_ready(const rtw_ctx *c, uint64_t n, uint32_t samples) {
    if (c->pend.active) return RTW_E_INVALID;
    if (!c->has_scene) return RTW_E_NO_SCENE;
    if (c->light_rows.empty()) return RTW_E_INVALID;
    if (n * c->light_rows.size() * samples > 0xFFFFFFFFull) return RTW_E_INVALID;
    return RTW_OK;
}

uint32_t rtw_ctx_light_count(const rtw_ctx *c) { return c ? (uint32_t)c->light_rows.size() : 0u; }

// The arguments of a launch over n points and [lo, hi]: views, sampling, and the light table, staged from the context's rows
static DirectArgs direct_args(const rtw_ctx *c, Staging &st, uint32_t n, uint32_t samples, uint32_t seed, float time, float lo, float hi, uint32_t accel) {
    DirectArgs a;
    fused_args(c, n, samples, seed, time, lo, hi, accel, a);
    a.n_lights = (uint32_t)c->light_rows.size();
    a.lights = st.in(c->light_rows.data(), sizeof(DirectRow) * c->light_rows.size());
    return a;
}

int rtw_ctx_direct_light(rtw_ctx *c, const float *points, const float *normals, uint32_t n, uint32_t samples, uint32_t seed, float time, float lo,
                         float hi, uint32_t accel, float *vis_out, float *irr_out, RtwStats *stats) {
    if (!c || !points || !normals || !vis_out || n == 0 || !ao_samples_ok(samples) || accel > RTW_ACCEL_BVH) return RTW_E_INVALID;
    if (const int rc = direct_ready(c, n, samples)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const bool tree = query_uses_tree(c, accel, time, lo, hi);

    Staging st(c);
    DirectArgs a = direct_args(c, st, n, samples, seed, time, lo, hi, accel);
    const size_t v_bytes = 3 * sizeof(float) * (size_t)n, o_bytes = sizeof(float) * (size_t)n * a.n_lights;
    a.points = st.in(points, v_bytes);
    a.normals = st.in(normals, v_bytes);
    a.vis_out = st.out(vis_out, o_bytes);
    if (irr_out) a.irr_out = st.out(irr_out, o_bytes);
    return counted_pass(c, st, 1, 0, stats, [&] { launch_direct_light(a, false, tree, c->stream); });
}

// depth_pass, then the direct-lighting kernel's camera form over its outputs
int rtw_ctx_direct_light_map(rtw_ctx *c, const RtwCamera *cam, uint32_t width, uint32_t height, float time, float mint, float maxt,
                             uint32_t samples, uint32_t seed, float lo, float hi, uint32_t accel, float *vis_out, float *irr_out,
                             float *depth_out, int32_t *idx_out, float *normal_out, RtwStats *stats) {
    if (!c || !cam || !vis_out || width == 0 || height == 0 || !ao_samples_ok(samples) || accel > RTW_ACCEL_BVH) return RTW_E_INVALID;
    if ((uint64_t)width * height > 0xFFFFFFFFull) return RTW_E_INVALID;
    if (const int rc = direct_ready(c, (uint64_t)width * height, samples)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t n = width * height;
    const bool tree = query_uses_tree(c, accel, time, mint, maxt), light_tree = query_uses_tree(c, accel, time, lo, hi);

    Staging st(c);
    DirectArgs a = direct_args(c, st, n, samples, seed, time, lo, hi, accel);
    const size_t o_bytes = sizeof(float) * (size_t)n * a.n_lights;
    a.vis_out = st.out(vis_out, o_bytes);
    if (irr_out) a.irr_out = st.out(irr_out, o_bytes);
    const QueryArgs q = depth_pass(c, st, cam, width, height, time, mint, maxt, accel, depth_out, idx_out, normal_out, a);
    return counted_pass(c, st, 1, n, stats, [&] { launch_scene_hits(q, true, tree, c->stream); },
                        [&] { launch_direct_light(a, true, light_tree, c->stream); });
}

int rtw_perlin_eval(const RtwPerlin *t, const float *points, uint32_t n, uint32_t turb_depth, float *out) {
    if (!t || !points || !out || n == 0) return RTW_E_INVALID;
    for (uint32_t i = 0; i < n; i++) out[i] = perlin_eval(*t, points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2], turb_depth);
    return RTW_OK;
}

int rtw_ctx_perlin_eval(rtw_ctx *c, const RtwPerlin *t, const float *points, uint32_t n, uint32_t turb_depth, float *out) {
    if (!c || !t || !points || !out || n == 0) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    Staging st(c, true);
    const RtwPerlin *d_t = st.in(t, sizeof(RtwPerlin));
    const float *d_p = st.in(points, 3 * sizeof(float) * (size_t)n);
    float *d_o = st.out(out, sizeof(float) * (size_t)n);
    if (st.e == hipSuccess) {
        launch_perlin_eval(d_t, d_p, n, turb_depth, d_o, c->stream);
        st.e = hipGetLastError();
    }
    return st.finish();
}

// The bilateral post-process (rtw_filter.hip) on this context's GPU and stream; the scene is not involved.
int rtw_ctx_bilateral_filter(rtw_ctx *c, const void *in, uint32_t w, uint32_t h, const RtwBilateral *p, uint8_t *out, RtwFilterStats *stats) {
    if (!c) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    return bilateral_filter_device(c->device, c->stream, &c->filter, in, w, h, p, out, stats, &g_last_hip);
}

// The guided filter (rtw_filter.hip) likewise.
int rtw_ctx_guided_filter(rtw_ctx *c, const void *in, uint32_t w, uint32_t h, const float *depth, const float *normal, const int32_t *idx,
                          const RtwGuidedFilter *p, uint8_t *out, RtwFilterStats *stats) {
    if (!c) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    return guided_filter_device(c->device, c->stream, &c->filter, c->opt_guided_layout, in, w, h, depth, normal, idx, p, out, stats, &g_last_hip);
}

// The a-trous filter (rtw_atrous.hip) likewise.
int rtw_ctx_atrous_filter(rtw_ctx *c, const float *in, uint32_t w, uint32_t h, const float *depth, const float *normal, const int32_t *idx,
                          const float *albedo, const float *emitted, const RtwAtrous *p, float *out, RtwFilterStats *stats) {
    if (!c) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    return atrous_filter_device(c->device, c->stream, &c->atrous, c->opt_atrous_layout, in, w, h, depth, normal, idx, albedo, emitted, p, out,
                                stats, &g_last_hip);
}

// The temporal accumulation (rtw_temporal.hip) likewise.
int rtw_ctx_temporal_accumulate(rtw_ctx *c, const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth, const float *normal,
                                const int32_t *idx, const RtwCamera *prev_cam, const float *prev_color, const float *prev_moments,
                                const float *prev_len, const float *prev_depth, const float *prev_normal, const int32_t *prev_idx,
                                const RtwTemporal *p, float *out_color, float *out_moments, float *out_len, float *out_variance,
                                RtwFilterStats *stats) {
    if (!c) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    const TemporalBuffers b = { cur, depth, normal, idx, prev_color, prev_moments, prev_len, prev_depth, prev_normal, prev_idx,
                                out_color, out_moments, out_len, out_variance };
    return temporal_accumulate_device(c->device, c->stream, &c->temporal, w, h, cam, prev_cam, b, p, nullptr, nullptr, nullptr, stats, &g_last_hip);
}

// ... and with moving objects (rtw.h "temporal accumulation with moving objects"): without rows and prev_xy the same launch
int rtw_ctx_temporal_accumulate_motion(rtw_ctx *c, const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth, const float *normal,
                                       const int32_t *idx, const RtwCamera *prev_cam, const float *prev_color, const float *prev_moments,
                                       const float *prev_len, const float *prev_depth, const float *prev_normal, const int32_t *prev_idx,
                                       const RtwTemporal *p, const RtwMotionRow *rows, uint32_t n_rows, uint32_t first, float *out_color,
                                       float *out_moments, float *out_len, float *out_variance, float *out_prev_xy, RtwFilterStats *stats) {
    if (!c) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    const TemporalBuffers b = { cur, depth, normal, idx, prev_color, prev_moments, prev_len, prev_depth, prev_normal, prev_idx,
                                out_color, out_moments, out_len, out_variance };
    const TemporalMotion m = { rows, n_rows, first, out_prev_xy };
    return temporal_accumulate_device(c->device, c->stream, &c->temporal, w, h, cam, prev_cam, b, p, &m, nullptr, nullptr, stats, &g_last_hip);
}

// ... and with per-pixel previous points (rtw.h "temporal accumulation with per-pixel motion"): without them the same launches
int rtw_ctx_temporal_accumulate_points(rtw_ctx *c, const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth, const float *normal,
                                       const int32_t *idx, const RtwCamera *prev_cam, const float *prev_color, const float *prev_moments,
                                       const float *prev_len, const float *prev_depth, const float *prev_normal, const int32_t *prev_idx,
                                       const RtwTemporal *p, const RtwMotionRow *rows, uint32_t n_rows, uint32_t first, const float *prev_point,
                                       const float *carried_normal, float *out_color, float *out_moments, float *out_len, float *out_variance,
                                       float *out_prev_xy, RtwFilterStats *stats) {
    if (!c) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    const TemporalBuffers b = { cur, depth, normal, idx, prev_color, prev_moments, prev_len, prev_depth, prev_normal, prev_idx,
                                out_color, out_moments, out_len, out_variance };
    const TemporalMotion m = { rows, n_rows, first, out_prev_xy };
    const TemporalPoints pt = { prev_point, carried_normal };
    return temporal_accumulate_device(c->device, c->stream, &c->temporal, w, h, cam, prev_cam, b, p, &m, &pt, nullptr, stats, &g_last_hip);
}

// ... and with bounds on the history's colour (rtw.h "bounded temporal accumulation"): without them the same launches
int rtw_ctx_temporal_accumulate_bounded(rtw_ctx *c, const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth,
                                        const float *normal, const int32_t *idx, const RtwCamera *prev_cam, const float *prev_color,
                                        const float *prev_moments, const float *prev_len, const float *prev_depth, const float *prev_normal,
                                        const int32_t *prev_idx, const RtwTemporal *p, const RtwMotionRow *rows, uint32_t n_rows, uint32_t first,
                                        const float *prev_point, const float *carried_normal, const float *hist_lo, const float *hist_hi,
                                        float *out_color, float *out_moments, float *out_len, float *out_variance, float *out_prev_xy,
                                        float *out_clipped, RtwFilterStats *stats) {
    if (!c) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    const TemporalBuffers b = { cur, depth, normal, idx, prev_color, prev_moments, prev_len, prev_depth, prev_normal, prev_idx,
                                out_color, out_moments, out_len, out_variance };
    const TemporalMotion m = { rows, n_rows, first, out_prev_xy };
    const TemporalPoints pt = { prev_point, carried_normal };
    const TemporalBounds bd = { hist_lo, hist_hi, out_clipped };
    return temporal_accumulate_device(c->device, c->stream, &c->temporal, w, h, cam, prev_cam, b, p, &m, &pt, &bd, stats, &g_last_hip);
}

// The motion rows of moved placements (rtw_mesh_move.hip) on this context's GPU and stream; the scene is not involved.
int rtw_ctx_mesh_instance_motion(rtw_ctx *c, const float *prev_poses, const float *cur_poses, uint32_t n, RtwMotionRow *rows_out, uint32_t *n_invalid) {
    if (!c || !prev_poses || !cur_poses || !rows_out || n == 0 || n > RTW_MAX_MESH_INSTANCES) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    MotionMem &m = c->motion_mem;
    const size_t pose_bytes = MOVE_POSE_BYTES * (size_t)n, row_bytes = sizeof(RtwMotionRow) * (size_t)n;
    HIP_TRY(m.bad.reserve(sizeof(uint32_t)));
    HIP_TRY(m.h_bad.reserve(sizeof(uint32_t)));
    const float *d_prev = prev_poses, *d_cur = cur_poses;
    RtwMotionRow *d_rows = rows_out;
    hipError_t e = hipSuccess;
    if (!on_device(prev_poses, c->device)) {
        HIP_TRY(m.prev.reserve(pose_bytes));
        e = hipMemcpyAsync(m.prev.ptr, prev_poses, pose_bytes, hipMemcpyDefault, c->stream);
        d_prev = m.prev.as<const float>();
    }
    if (e == hipSuccess && !on_device(cur_poses, c->device)) {
        HIP_TRY(m.cur.reserve(pose_bytes));
        e = hipMemcpyAsync(m.cur.ptr, cur_poses, pose_bytes, hipMemcpyDefault, c->stream);
        d_cur = m.cur.as<const float>();
    }
    if (!on_device(rows_out, c->device)) {
        HIP_TRY(m.rows.reserve(row_bytes));
        d_rows = m.rows.as<RtwMotionRow>();
    }
    if (e == hipSuccess) e = hipMemsetAsync(m.bad.ptr, 0, sizeof(uint32_t), c->stream);
    if (e == hipSuccess) {
        launch_mesh_motion(d_prev, d_cur, n, d_rows, m.bad.as<uint32_t>(), c->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess && d_rows != rows_out) e = hipMemcpyAsync(rows_out, d_rows, row_bytes, hipMemcpyDefault, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(m.h_bad.ptr, m.bad.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (const int rc = call_status(c, e)) return rc;
    if (n_invalid) *n_invalid = *m.h_bad.as<uint32_t>();
    return RTW_OK;
}

// Previous points of a deformed mesh (rtw_mesh_move.hip) on this context's GPU and stream; the scene is not involved: the
// caller kept prev_ouv (and prev_poses) from the previous frame.
int rtw_ctx_deform_motion(rtw_ctx *c, const int32_t *tri, const float *bary, uint32_t n, const float *prev_ouv, uint32_t n_tris, const int32_t *idx,
                          const float *prev_poses, uint32_t n_mesh, uint32_t first, float *prev_point_out, float *carried_normal_out) {
    DeformMesh m = { prev_ouv, n_tris, idx, prev_poses, prev_poses ? n_mesh : 0u, prev_poses ? first : 0u };
    if (!c || !deform_args_ok(tri, bary, n, m, prev_point_out, carried_normal_out)) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    DeformMem &dm = c->deform_mem;
    if (!prev_poses) m.idx = nullptr;
    const size_t f1 = sizeof(float) * (size_t)n;
    hipError_t e = hipSuccess;
    struct Stage { const void **p; DevMem *mem; size_t bytes; };
    const Stage stages[5] = { { (const void **)&tri, &dm.tri, sizeof(int32_t) * (size_t)n },
                              { (const void **)&bary, &dm.bary, 2 * f1 },
                              { (const void **)&m.prev_ouv, &dm.ouv, 9 * sizeof(float) * (size_t)n_tris },
                              { (const void **)&m.idx, &dm.idx, sizeof(int32_t) * (size_t)n },
                              { (const void **)&m.prev_poses, &dm.poses, MOVE_POSE_BYTES * (size_t)m.n_mesh } };
    for (const Stage &st : stages) {
        if (!*st.p || on_device(*st.p, c->device)) continue;
        HIP_TRY(st.mem->reserve(st.bytes));
        if (e == hipSuccess) e = hipMemcpyAsync(st.mem->ptr, *st.p, st.bytes, hipMemcpyDefault, c->stream);
        *st.p = st.mem->ptr;
    }
    float *d_point = prev_point_out, *d_normal = carried_normal_out;
    if (!on_device(prev_point_out, c->device)) { HIP_TRY(dm.point.reserve(3 * f1)); d_point = dm.point.as<float>(); }
    if (!on_device(carried_normal_out, c->device)) { HIP_TRY(dm.normal.reserve(3 * f1)); d_normal = dm.normal.as<float>(); }
    if (e == hipSuccess) {
        launch_deform_motion(tri, bary, n, m, d_point, d_normal, c->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess && d_point != prev_point_out) e = hipMemcpyAsync(prev_point_out, d_point, 3 * f1, hipMemcpyDefault, c->stream);
    if (e == hipSuccess && d_normal != carried_normal_out) e = hipMemcpyAsync(carried_normal_out, d_normal, 3 * f1, hipMemcpyDefault, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return call_status(c, e);
}

// The variance estimate and the variance-steered a-trous filter (rtw_svgf.hip) likewise, on the a-trous filter's scratch.
int rtw_ctx_variance_estimate(rtw_ctx *c, const float *moments, const float *len, uint32_t w, uint32_t h, const float *depth, const float *normal,
                              const int32_t *idx, const RtwVarianceEstimate *p, float *out, RtwFilterStats *stats) {
    if (!c) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    return variance_estimate_device(c->device, c->stream, &c->atrous, c->opt_atrous_layout, moments, len, w, h, depth, normal, idx, p, out, stats,
                                    &g_last_hip);
}

int rtw_ctx_svgf_filter(rtw_ctx *c, const float *in, const float *variance, uint32_t w, uint32_t h, const float *depth, const float *normal,
                        const int32_t *idx, const float *albedo, const float *emitted, const RtwAtrous *p, const RtwSvgf *vp, float *out,
                        float *out_variance, RtwFilterStats *stats) {
    if (!c) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    return svgf_filter_device(c->device, c->stream, &c->atrous, c->opt_atrous_layout, in, variance, w, h, depth, normal, idx, albedo, emitted, p, vp,
                              out, out_variance, stats, &g_last_hip);
}

// The neighbourhood colour bounds (rtw_bounds.hip) likewise, on a scratch of their own.
int rtw_ctx_colour_bounds(rtw_ctx *c, const float *in, uint32_t w, uint32_t h, const int32_t *idx, const RtwColourBounds *p, float *out_lo,
                          float *out_hi, float *out_clamped, RtwFilterStats *stats) {
    if (!c) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    return colour_bounds_device(c->device, c->stream, &c->bounds, c->opt_atrous_layout, in, w, h, idx, p, out_lo, out_hi, out_clamped, stats,
                                &g_last_hip);
}

// The guide-steered upsampling (rtw_upsample.hip) likewise, on a scratch of its own.
int rtw_ctx_upsample_filter(rtw_ctx *c, const float *lo, uint32_t w_lo, uint32_t h_lo, const RtwGuides *guides_lo, uint32_t w, uint32_t h,
                            const RtwGuides *guides_hi, const RtwUpsample *p, float *out, float *wsum_out, RtwFilterStats *stats) {
    if (!c) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    return upsample_filter_device(c->device, c->stream, &c->upsample, c->opt_atrous_layout, lo, w_lo, h_lo, guides_lo, w, h, guides_hi, p, out,
                                  wsum_out, stats, &g_last_hip);
}

// The display stage (rtw_display.hip) likewise, on a scratch of its own.
int rtw_ctx_luminance_histogram(rtw_ctx *c, const float *in, uint32_t w, uint32_t h, uint32_t *hist, uint32_t *counts, RtwFilterStats *stats) {
    if (!c) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    return luminance_histogram_device(c->device, c->stream, &c->display, c->opt_histogram_count, in, w, h, hist, counts, stats, &g_last_hip);
}

int rtw_ctx_display(rtw_ctx *c, const float *in, uint32_t w, uint32_t h, const RtwDisplay *p, void *out, RtwFilterStats *stats) {
    if (!c) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    return display_device(c->device, c->stream, &c->display, in, w, h, p, out, stats, &g_last_hip);
}

// Bloom (rtw_bloom.hip) likewise, on a scratch of its own.
int rtw_ctx_bloom(rtw_ctx *c, const float *in, uint32_t w, uint32_t h, const RtwBloom *p, float *out, float *layer_out, RtwFilterStats *stats) {
    if (!c) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    return bloom_device(c->device, c->stream, &c->bloom, c->opt_atrous_layout, in, w, h, p, out, layer_out, stats, &g_last_hip);
}

// The device-math probe (rtw_probe.hip, rtw.h "device math, for tests") on this context's GPU and stream; the scene is not involved.
int rtw_ctx_device_math(rtw_ctx *c, uint32_t fn, const float *in, uint32_t n_cols, uint32_t n, float *out, uint32_t out_cols) {
    if (!c) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    return device_math_device(c->device, c->stream, fn, in, n_cols, n, out, out_cols, &g_last_hip);
}
int rtw_ctx_device_sweep(rtw_ctx *c, uint32_t which, uint64_t first, uint64_t count, uint32_t seed, RtwSweepResult *result) {
    if (!c) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    return device_sweep_device(c->device, c->stream, which, first, count, seed, result, &g_last_hip);
}

} // extern "C"

// Copy the compact rows of partition (row_block, part_index, part_count) from `src` (device) to their image rows of the
// full frame `dst` (host, or device memory of any GPU): the blocks a partition owns are equally spaced in the frame, so ONE
// strided 2-D copy moves all the full blocks, and a second, 1-D, the ragged last block when this partition owns it.
static int scatter_rows(rtw_ctx *c, const float *src, float *dst, uint32_t width, uint32_t height, uint32_t row_block,
                        uint32_t part_index, uint32_t part_count) {
    const size_t row_bytes = (size_t)width * 3 * sizeof(float);
    if (part_count <= 1) { HIP_TRY(hipMemcpyAsync(dst, src, row_bytes * height, hipMemcpyDefault, c->stream)); return RTW_OK; }
    const uint32_t n_blocks = (height + row_block - 1) / row_block;
    uint32_t mine = 0, full = 0;                                    // blocks b = part_index + k * part_count < n_blocks
    if (part_index < n_blocks) mine = (n_blocks - 1 - part_index) / part_count + 1;
    const bool ragged = height % row_block != 0;
    const bool own_last = mine > 0 && (part_index + (mine - 1) * part_count) == n_blocks - 1;
    full = mine - ((ragged && own_last) ? 1u : 0u);
    const size_t block_bytes = row_bytes * row_block;
    if (full) HIP_TRY(hipMemcpy2DAsync((char *)dst + (size_t)part_index * block_bytes, (size_t)part_count * block_bytes, src, block_bytes,
                                       block_bytes, full, hipMemcpyDefault, c->stream));
    if (full < mine) {
        const uint32_t b = part_index + full * part_count;
        HIP_TRY(hipMemcpyAsync((char *)dst + (size_t)b * block_bytes, (const char *)src + (size_t)full * block_bytes,
                               row_bytes * (height - b * row_block), hipMemcpyDefault, c->stream));
    }
    return RTW_OK;
}

// ... the same on the host, from the pinned staging buffer into a pageable frame (render_wait)
static void scatter_rows_host(const float *src, float *dst, uint32_t width, uint32_t height, uint32_t n_rows, uint32_t row_block, uint32_t part_index, uint32_t part_count) {
    const size_t row_floats = (size_t)width * 3;
    if (part_count <= 1) { std::memcpy(dst, src, row_floats * height * sizeof(float)); return; }
    for (uint32_t k = 0; k < n_rows; k += row_block) {               // compact rows [k, k + rows) are image rows [j, j + rows)
        const uint32_t j = ((k / row_block) * part_count + part_index) * row_block;
        const uint32_t rows = std::min(row_block, std::min(n_rows - k, height - j));
        std::memcpy(dst + (size_t)j * row_floats, src + (size_t)k * row_floats, rows * row_floats * sizeof(float));
    }
}

// A render is three phases: PREPARE (argument checks, first-use allocations, driver queries: may wait for the device), LAUNCH (memsets, kernels,
// events, counter read-back: never waits), COPY (the rows toward the caller's memory: never waits for the device either -- a pageable multi-GPU
// host frame is staged through pinned memory and finished on the host in render_wait).  rtw_ctx_render runs them back to back; rtw_mgpu_render
// runs each phase for EVERY device before the next phase for any, so that no device's work is held up by another's.
enum : unsigned { PH_PREPARE = 1u, PH_LAUNCH = 2u, PH_COPY = 4u, PH_ALL = 7u };
static int render_enqueue_impl(rtw_ctx *c, const RtwCamera *cam, const RtwParams *p, OutSpec out, unsigned phases);
static int render_copy(rtw_ctx *c);

// Launch one render on the context's stream; nothing here waits for the GPU (apart from a first-use hipMalloc).  On failure nothing of
// this call is left running: whatever was already launched is waited for, so the caller may free or reuse its buffers at once.
static int render_enqueue(rtw_ctx *c, const RtwCamera *cam, const RtwParams *p, OutSpec out, unsigned phases = PH_ALL) {
    const int rc = render_enqueue_impl(c, cam, p, out, phases);
    if (rc != RTW_OK && c && c->stream && !c->pend.active) {
        const int keep = g_last_hip;
        if (hipStreamSynchronize(c->stream) != hipSuccess) (void)hipGetLastError();
        g_last_hip = keep;
    }
    return rc;
}

// The build a render runs and its dynamic LDS, from plain facts: what the request needs, what the tree allows, the kernel of the two
// (rtw_host.h, rtw_kernels.h), each asked once.  fn is null when no such build is compiled.  Shared with rtw_render_choice.
struct RenderChoice { RenderBuild build; LdsLayout lds; render_fn fn; };
static RenderChoice render_choice(const RtwRenderFacts &f, const RtwTreeFacts &t, int opt_lds_geom, uint32_t opt_node_format, bool moving, bool bvh) {
    const RenderNeed need = render_need(f);
    const bool large = render_block(RenderBuild{ true, moving, need.geom, 1, need.spec }) != RTW_BLOCK;      // its NODES == 1 build walks f32 planes
    const LdsLayout lds = render_lds_layout(t, opt_lds_geom, opt_node_format, bvh, (f.flags & RTW_FLAG_GLOBAL_NODES) != 0u, need.geom, large, f.n_triangles != 0u);
    const RenderBuild build{ bvh, moving, need.geom, lds.nodes, need.spec };
    const render_fn fn = render_kernel(build);
    return RenderChoice{ build, lds, fn && render_block(build) == lds.block ? fn : nullptr };
}

// The work queue of one band as its launch was handed it (rtw_ctx_last_queue_plan): copies of KArgs' fields, nothing computed again.
static RtwQueuePlan queue_plan(const KArgs &a, uint32_t grid, uint32_t block) {
    RtwQueuePlan q;
    std::memset(&q, 0, sizeof q);
    q.n_tiles = a.n_tiles; q.tiles_x = a.tiles_x; q.k_base = a.k_base; q.k_end = a.k_end;
    q.n_samples = a.n_samples; q.chunk_len = a.chunk_len; q.n_chunks = a.n_chunks; q.bank_len = a.bank_len;
    q.reg_q1 = a.reg_q1; q.reg_q2 = a.reg_q2;
    for (int r = 0; r < 3; r++) { q.reg_len[r] = a.reg_len[r]; q.reg_nc[r] = a.reg_nc[r]; }
    q.total_work = a.total_work;
    q.sub_shift = a.sub_shift; q.grab_shift = a.grab_shift; q.grab_max = a.grab_max;
    q.grid = grid; q.block = block;
    q.has_tile_order = a.tile_order ? 1u : 0u;
    q.row_block = a.row_block; q.part_index = a.part_index; q.part_count = a.part_count;
    return q;
}

static int render_enqueue_impl(rtw_ctx *c, const RtwCamera *cam, const RtwParams *p, OutSpec out, unsigned phases) {
    if (!c || !cam || !p || !out.base) return RTW_E_INVALID;
    if (c->pend.active) return RTW_E_INVALID;
    if (!c->has_scene) return RTW_E_NO_SCENE;
    if (p->width == 0 || p->height == 0 || p->samples == 0) return RTW_E_INVALID;
    if (p->integrator > RTW_INTEGRATOR_LIGHT_BIASED || p->sampler > RTW_SAMPLER_NO_RAND || p->accel > RTW_ACCEL_BVH) return RTW_E_INVALID;
    if (p->part_count > 1 && (p->row_block == 0 || p->part_index >= p->part_count)) return RTW_E_INVALID;
    if (p->width > 65535u || p->height > 65535u) return RTW_E_INVALID;      // a lane keeps (column, row) in one register (rtw_kernels.hip Pixel)
    if (const int qrc = quats_render_check(c->inst_quats != nullptr, p->integrator, c->noise_active, c->tris.n != 0u)) return qrc;
    if (const int prc = mesh_render_check(c->mesh_rows != nullptr, p->integrator, (p->flags & RTW_FLAG_MIXED_MATERIAL) && c->has_mixed, c->inst_quats != nullptr)) return prc;
    if (c->noise_active && p->integrator == RTW_INTEGRATOR_RUST2) return RTW_E_UNSUPPORTED;   // Rust2's textures have no noise
    if (c->noise_active && c->tris.n) return RTW_E_UNSUPPORTED;                              // (rtw_ctx_set_triangles / _set_texture_noise refuse it too)
    const bool light_integrator = p->integrator == RTW_INTEGRATOR_LIGHT_CAST || p->integrator == RTW_INTEGRATOR_LIGHT_BIASED;
    // Rust2's light-biased integrators: no noise (Rust2's textures have none), no triangle lights or occluders yet, no media (Rust2 has none)
    if (light_integrator && (c->noise_active || c->tris.n || c->has_medium)) return RTW_E_UNSUPPORTED;
    // RTW_FLAG_MIXED_MATERIAL: Rust2's integrators only; a scene with a MixedMaterial object runs the mixed build, which is the light build's driver
    if (const int mrc = mixed_check(p->flags, p->integrator, c->has_mixed, c->mixed_bad, c->noise_active, c->tris.n != 0u, c->has_medium)) return mrc;
    const bool mixed_active = (p->flags & RTW_FLAG_MIXED_MATERIAL) && c->has_mixed;
    if (!c->pend.marked) c->pend.t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(c->device));

    // The BVH's pruning is proven against the reference's ROUNDED quadratic (DESIGN.md "Conservative traversal"), which presumes
    // that d.d is an ordinary f32.  Scattered directions are unit-scale by construction; camera directions are whatever the caller's
    // camera says (the reference never normalises them), and when |d|^2 can overflow or underflow f32 the reference's quadratic
    // degenerates -- NaN roots pass both range tests and are reported as hits (sphere.rs:118-121) -- which only the list walk
    // reproduces.  Bound |d| over the image from the camera (d = pixel00 + x delta_u + y delta_v, x in [0,W], y in [0,H]):
    // above by the triangle inequality, below by the distance of that plane from the origin; outside [1e-15, 1e15] walk the list.
    uint32_t accel = p->accel;
    if (accel == RTW_ACCEL_BVH) {
        const double P[3] = { cam->pixel00[0], cam->pixel00[1], cam->pixel00[2] };
        const double U[3] = { cam->delta_u[0], cam->delta_u[1], cam->delta_u[2] }, V[3] = { cam->delta_v[0], cam->delta_v[1], cam->delta_v[2] };
        auto norm = [](const double *v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
        const double W = (double)p->width + 1.0, H = (double)p->height + 1.0;
        const double hi = norm(P) + W * norm(U) + H * norm(V);
        const double N[3] = { U[1] * V[2] - U[2] * V[1], U[2] * V[0] - U[0] * V[2], U[0] * V[1] - U[1] * V[0] };
        const double nn = norm(N);
        const double lo = nn > 0.0 ? std::fabs(P[0] * N[0] + P[1] * N[1] + P[2] * N[2]) / nn : 0.0;
        if (!(hi <= 1e15) || !(lo >= 1e-15)) accel = RTW_ACCEL_BRUTE;
        // ... and that the origin is one: past 2^60 (or NaN) the squares of the quadratic overflow and the same NaN roots appear
        const double O[3] = { cam->origin[0], cam->origin[1], cam->origin[2] }, CU[3] = { cam->u[0], cam->u[1], cam->u[2] }, CV[3] = { cam->v[0], cam->v[1], cam->v[2] };
        if (!(norm(O) + std::fabs((double)cam->lens_radius) * (norm(CU) + norm(CV)) <= 0x1p60)) accel = RTW_ACCEL_BRUTE;
        // ... and that the scene is one (rtw_ctx_set_scene: scene_span): b = oc . d and a c = (d . d)(oc . oc - r^2) must stay below f32's 3.4e38, so
        // |d| x (the farthest centre + the camera's distance) is kept below 1e18 (camera rays: `hi` above; scattered rays are unit-scale)
        if (!(std::fmax(hi, 2.0) * (c->scene_span + norm(O) + 1.0) <= 1e18)) accel = RTW_ACCEL_BRUTE;
        // ... and the accepted range: with a NaN bound the reference's `x < mint || x > maxt` rejects nothing, where the tree's interval test rejects everything
        if (p->mint != p->mint || p->maxt != p->maxt) accel = RTW_ACCEL_BRUTE;
        // The tree's bounds cover ray.time in [t_begin, t_end] only (rtw_ctx_set_scene): outside it a moving sphere can leave its box
        if (c->sc.moving) {
            const float ta = cam->time0, tb = cam->time0 + cam->shutter;
            if (!(std::fmin(ta, tb) >= c->t_begin && std::fmax(ta, tb) <= c->t_end)) accel = RTW_ACCEL_BRUTE;
            if (ta != ta || tb != tb) accel = RTW_ACCEL_BRUTE;         // (fmin / fmax drop a NaN: a NaN shutter makes every moving centre NaN, which only the list walk answers like the reference)
            if ((light_integrator || mixed_active) && !(c->t_begin <= 0.0f && c->t_end >= 0.0f)) accel = RTW_ACCEL_BRUTE;   // the shadow rays run at ray.time 0, and so do the rays a MixedMaterial scatters
        }
        if (!c->bvh_ok) accel = RTW_ACCEL_BRUTE;
        // a handful of spheres: the list walk IS the fastest closest-hit (the traversal scheduler only costs)
        if (c->sc.n <= c->opt_list_walk_max) accel = RTW_ACCEL_BRUTE;
    }

    KArgs a;
    std::memset(&a, 0, sizeof a);
    a.cam = *cam; a.sc = c->sc; a.bvh = c->bvh; a.geom = c->geom;
    if (p->flags & RTW_FLAG_GLOBAL_NODES) a.bvh.nodes16 = nullptr;
    a.flags = p->flags;
    if (!mixed_active) a.flags &= ~RTW_FLAG_MIXED_MATERIAL;       // (the bit selects the mixed build: render_need; without a MixedMaterial object every build is as it was)
    a.width = p->width; a.height = p->height;
    const uint32_t n_rows = rtw_part_rows(p->height, p->row_block, p->part_index, p->part_count);
    a.row_block = p->row_block ? p->row_block : 1; a.part_index = p->part_index; a.part_count = p->part_count;
    a.tiles_x = (p->width + 7) / 8;
    a.n_samples = sampler_count(p->sampler, p->samples, &a.s_root);
    if (a.n_samples == 0 || a.n_samples >= (1u << 24)) return RTW_E_INVALID;   // (sample index and samples left in the unit share a register)
    a.sampler = p->sampler; a.integrator = p->integrator; a.depth = p->depth;
    a.has_textures = c->has_textures ? 1u : 0u;
    a.seed_lo = (uint32_t)p->seed; a.seed_hi = (uint32_t)(p->seed >> 32);
    a.inv_gamma = host_div(1.0f, p->gamma);                       // viewport.rs:232
    a.mint = p->mint; a.maxt = p->maxt;
    std::memcpy(a.bg, c->bg, sizeof a.bg);
    a.queue = c->scr.queue.as<uint32_t>(); a.stats = c->scr.stats.as<unsigned long long>();
    if (c->noise_active) a.noise = c->noise;                       // (selects the noise build: render_need)
    if (c->tris.n) a.tris = tri_view(c, p->accel, p->mint, p->maxt);   // (selects the triangle build; the tree for RTW_ACCEL_BVH requests)
    if (light_integrator) a.lights = c->lights;                    // (the integrator selects the light build, which alone reads them)
    a.inst_quats = c->inst_quats;                                  // (selects the quaternion build, whatever the integrator of the three it serves)
    a.mesh_rows = c->mesh_rows; a.n_mesh = c->n_mesh;              // (selects the placement build)
    if (c->mesh_rows) { a.mesh_top = mesh_top_view(c, a.tris); a.n_mesh_top = c->n_mesh_top; }   // (the same build: the walk behind the pointer)
#ifdef RTW_ENDTIMES
    if (const char *e = getenv("RTW_ENDTIMES_REF")) a.endtimes_ref = std::strtoull(e, nullptr, 10);       // diagnostic build only
#endif

    // Work units are (tile, chunk of samples, pixel): a pixel's samples are spread over ceil(n / chunk_len) units
    // so that no lane owns more than chunk_len sequential paths (the slowest PIXEL used to set a ~50 ms tail).
    // Every sample's radiance is banked in HBM and added in order by resolve_kernel: 12 B per camera ray
    // (12.4 GB for 1920x1080x500) -- the image is rendered in bands of tile rows when that exceeds the budget.
    // RTW_FLAG_CHUNK_SUMS banks one partial sum per unit instead (bank_len = 1: one slot per unit and pixel).
    const bool sums = (p->flags & RTW_FLAG_CHUNK_SUMS) != 0;
    uint32_t chunk_len = (p->flags & RTW_FLAG_CHUNK_SUMS) ? RTW_SUM_CHUNK : c->opt_chunk_len;   // (the summation chunk is part of the image's definition)
    if (chunk_len == 0) {
        // auto: the unit length follows the size of the launch (profiles/r02_order_chunk_grid.log).  Long units amortise the per-unit work
        // (queue, pixel hash, bank addressing) but lengthen the tail of the launch, which is one unit deep: the whole bench frame
        // (660 units of 4 per lane) runs in 101.0 / 98.5 / 97.4 ms with units of 4 / 6 / 8, an eighth of it (82 per lane) in 13.46 /
        // 13.34 / 13.55, C2 (51 per lane) in 8.97 / 9.17 / 9.37.  A frame so small that one workgroup per CU is enough (below) gets
        // units of 2 (C1: 0.276 -> 0.261 ms).
        const uint64_t units4 = (uint64_t)a.tiles_x * ((n_rows + 7) / 8) * ((a.n_samples + 3) / 4) * 64ull;
        const uint64_t lanes = (uint64_t)c->n_cu * 1536ull;       // 24 resident waves per CU (6 per SIMD: the register budget of the specialised builds)
        // (units of 12 from 500 per lane: bench frame 97.8 -> 97.0 ms, C4 386.1 -> 383.7; 16..32 gain C4 another 0.6 % and lose the bench frame 0.3..0.9 %)
        chunk_len = units4 >= 500ull * lanes ? 12u : units4 >= 200ull * lanes ? 8u : units4 >= 64ull * lanes ? 6u : (units4 * 6ull < 16ull * lanes ? 2u : 4u);
    }
    if (chunk_len > a.n_samples) chunk_len = a.n_samples;
    a.chunk_len = chunk_len;
    a.n_chunks = (a.n_samples + chunk_len - 1) / chunk_len;
    a.bank_len = sums ? 1u : 0u;
    // the bank: one slot per (tile, sample, pixel) -- whatever the unit lengths --, or per (tile, unit, pixel) for the partial sums
    const uint64_t slots_per_tile_row = (uint64_t)a.tiles_x * (sums ? a.n_chunks : a.n_samples) * 64ull;
    uint64_t max_slots = c->opt_bank_bytes / 12; if (max_slots > 0xFFFFFFF0ull) max_slots = 0xFFFFFFF0ull;
    // (work items are counted in 32 bits as well: 64 per tile and unit, at most one unit per sample)
    const uint64_t items_per_tile_row = slots_per_tile_row;
    const uint32_t tile_rows = (n_rows + 7) / 8;
    uint64_t band_tile_rows = max_slots / (slots_per_tile_row ? slots_per_tile_row : 1);
    if (band_tile_rows > 0xFFFFFFF0ull / items_per_tile_row) band_tile_rows = 0xFFFFFFF0ull / items_per_tile_row;
    if (band_tile_rows == 0) return RTW_E_NOMEM;                  // one row of tiles does not fit the budget
    if (band_tile_rows > tile_rows) band_tile_rows = tile_rows;
    const size_t sample_bytes = (size_t)(band_tile_rows * slots_per_tile_row) * 12;
    if (c->scr.samples.reserve(sample_bytes) != hipSuccess) { (void)hipGetLastError(); return RTW_E_NOMEM; }
    a.samples = c->scr.samples.as<float>();

    // destination: the kernels write compact rows either straight into the caller's device buffer or into the context's
    const size_t out_bytes = (size_t)n_rows * p->width * 3 * sizeof(float);
    // (asked on every call, a few microseconds: the same address can be host memory in one call and device memory in the next)
    bool pinned_host = false;
    {
        hipPointerAttribute_t attr;
        c->attr_on_device = false; c->attr_device = -1;
        if (hipPointerGetAttributes(&attr, out.base) == hipSuccess) {
            c->attr_on_device = attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
            pinned_host = attr.type == hipMemoryTypeHost;          // hipHostMalloc / hipHostRegister: a copy into it is a true asynchronous DMA
            c->attr_device = attr.device;
        } else (void)hipGetLastError();
    }
    const bool direct = c->attr_on_device && c->attr_device == c->device && !(out.scatter && p->part_count > 1);
    // A multi-GPU frame in pageable host memory (the reference's Img, a Vec, a numpy array): staged through this context's pinned buffer
    const bool staged = out.scatter && !c->attr_on_device && !pinned_host;
    if (staged && c->scr.h_out.reserve(out_bytes) != hipSuccess) { (void)hipGetLastError(); return RTW_E_NOMEM; }
    if (direct) a.out = out.base;
    else {
        HIP_TRY(c->scr.out.reserve(out_bytes));
        a.out = c->scr.out.as<float>();
    }

    // The build this render runs and its dynamic LDS, chosen once: everything below -- the LDS allowance, the occupancy, the grid, the grabs,
    // the launch -- uses `build`, `fn` and `block`.
    RtwRenderFacts facts{};
    facts.integrator = a.integrator; facts.sampler = a.sampler; facts.depth = a.depth; facts.flags = a.flags; facts.has_textures = a.has_textures;
    facts.n_quads = a.geom.n_quads; facts.n_instances = a.geom.n_inst; facts.noise = a.noise.tex != nullptr; facts.n_triangles = a.tris.n;
    facts.rotations = a.inst_quats != nullptr; facts.placements = a.mesh_rows != nullptr;
    const RenderChoice choice = render_choice(facts, RtwTreeFacts{ c->bvh.n_nodes, c->bvh.depth, c->sc.n, c->bvh.nodes16 != nullptr, c->nodes32 != nullptr },
                                              c->opt_lds_geom, c->opt_node_format, c->sc.moving != 0, accel == RTW_ACCEL_BVH);
    if (!choice.fn) return RTW_E_UNSUPPORTED;          // (no such build: an error, never another kernel)
    const RenderBuild &build = choice.build;
    const LdsLayout &lds = choice.lds;
    const render_fn fn = choice.fn;
    const uint32_t block = lds.block;                  // threads per workgroup of the render kernel this launch runs
    a.lds_stack_off = lds.stack_off; a.lds_geom_off = lds.geom_off; a.lds_bytes = lds.bytes;
    if (a.tris.n) a.tris.lds_off = lds.tri_off;
    if (lds.node_format == 2u) a.nodes32 = c->nodes32;

    if (build.bvh && a.lds_bytes > 64u * 1024u) {
        // more than the 64 KiB a workgroup gets by default (a large workgroup's f32 planes and stack: Book-1 73.5 KB): allowed per kernel and device, once per size
        uint32_t &allowed = c->lds_allowed[(const void *)fn];
        if (allowed < a.lds_bytes) { HIP_TRY(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds_bytes)); allowed = a.lds_bytes; }
    }
    // persistent grid: as many workgroups as the kernel's registers let be resident, capped by the work
    uint32_t per_cu = c->opt_blocks_per_cu;
    if (per_cu == 0) {
        const auto key = std::make_pair((const void *)fn, a.lds_bytes);
        auto it = c->occupancy.find(key);
        if (it == c->occupancy.end()) {
            int n = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)fn, (int)block, a.lds_bytes) != hipSuccess || n < 1) n = 1;
            it = c->occupancy.emplace(key, (uint32_t)(n > 8 ? 8 : n)).first;
        }
        per_cu = it->second;
    }

    if (!(phases & PH_LAUNCH)) return RTW_OK;          // PREPARE only: everything that can wait for the device is behind us

    if (!c->pend.marked) HIP_TRY(hipEventRecord(c->ev_mark, c->stream));
    HIP_TRY(hipMemsetAsync(a.stats, 0, RTW_N_STATS * sizeof(unsigned long long), c->stream));
#ifdef RTW_ENDTIMES
    HIP_TRY(hipMemsetAsync(a.stats + 24, 0xFF, sizeof(unsigned long long), c->stream));     // atomicMin targets (diagnostic build only)
    HIP_TRY(hipMemsetAsync(a.stats + 26, 0xFF, sizeof(unsigned long long), c->stream));
    HIP_TRY(hipMemsetAsync(a.stats + 28, 0xFF, sizeof(unsigned long long), c->stream));
#endif
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    std::vector<RtwQueuePlan> plans;                   // what each band's launch is handed (rtw_ctx_last_queue_plan): kept once all are issued
    for (uint32_t tr0 = 0; tr0 < tile_rows || tr0 == 0; tr0 += (uint32_t)band_tile_rows) {
        const uint32_t tr1 = tr0 + (uint32_t)band_tile_rows < tile_rows ? tr0 + (uint32_t)band_tile_rows : tile_rows;
        a.k_base = tr0 * 8; a.k_end = tr1 * 8 < n_rows ? tr1 * 8 : n_rows;
        a.n_tiles = a.tiles_x * (tr1 - tr0);
        a.total_work = a.n_tiles * a.n_chunks * 64u;              // < 2^32 by the item bound above  (one region; refined below)
        a.reg_q1 = a.reg_q2 = a.n_tiles;
        for (int r = 0; r < 3; r++) { a.reg_len[r] = a.chunk_len; a.reg_nc[r] = a.n_chunks; }
        a.tile_order = nullptr;
        if (c->opt_tile_order && a.n_tiles > 2u && !((c->opt_tile_order == 2u || c->opt_tile_order == 5u) && c->cull.n_other)) {    // (quads / instances: no cost guess, raster order)
            // queue order of the tiles (rtw_host.cpp build_tile_order): built once per (mode, frame shape, camera, partition, scene), kept on the device
            const uint32_t tiles_y = a.n_tiles / a.tiles_x;
            TileOrderKey key;
            std::memset(&key, 0, sizeof key);
            key.mode = c->opt_tile_order; key.tiles_x = a.tiles_x; key.tiles_y = tiles_y; key.k_base = a.k_base;
            key.row_block = a.row_block; key.part_index = a.part_index; key.part_count = a.part_count; key.cam = *cam; key.scene_serial = c->scene_serial;
            key.cam.time0 = key.cam.shutter = key.cam.lens_radius = 0.0f;     // (the estimate uses the centre rays only: the frames of a clip share one order)
            // tiles worth of work in flight when the queue runs dry: four units for every lane of the full grid
            const uint64_t per_tile = 64ull * a.n_chunks;
            key.tail_tiles = (uint32_t)std::min<uint64_t>(a.n_tiles, ((uint64_t)c->n_cu * per_cu * block * 4ull + per_tile - 1) / per_tile);
            if (!c->scr.order.ptr || std::memcmp(&key, &c->order_key, sizeof key) != 0) {
                std::vector<uint32_t> order;
                build_tile_order(c->opt_tile_order, a.tiles_x, tiles_y, a.k_base, a.row_block, a.part_index, a.part_count, *cam, c->cull, key.tail_tiles, order);
                HIP_TRY(c->scr.order.reserve(order.size() * sizeof(uint32_t)));
                HIP_TRY(hipMemcpyAsync(c->scr.order.ptr, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));          // (`order` is a local: the copy must be done before it goes away; once per frame shape)
                c->order_key = key;
            }
            a.tile_order = c->scr.order.as<uint32_t>();
        }
        // Small launches are latency-bound, not throughput-bound: a lane should own >= ~16 work units before another resident
        // workgroup per CU pays (profiles/r02_small_frame.log: C1 0.494 -> 0.276 ms with 1 workgroup per CU instead of 6, `First
        // frame` 3.15 -> 2.68 ms with 4; the 1080p frames are indifferent).  An explicit RTW_OPT_BLOCKS_PER_CU wins.
        uint32_t wg_per_cu = per_cu;
        if (c->opt_blocks_per_cu == 0) {
            const uint64_t lanes_per_wg_row = (uint64_t)c->n_cu * block * 16ull;
            const uint64_t want = ((uint64_t)a.total_work + lanes_per_wg_row - 1) / lanes_per_wg_row;
            if (want < wg_per_cu) wg_per_cu = (uint32_t)(want ? want : 1);
            // The specialised BVH builds are compiled for 7 waves/SIMD (72 VGPRs); the seventh workgroup per CU pays on the full 1080p frames
            // (bench frame 77.9 -> 76.4 ms, C4 319 -> 311, C5 96.8 -> 95.0) and costs on shorter launches (an eighth of the bench frame 10.9 ->
            // 11.1 ms, C2 7.18 -> 7.35: one more wave per SIMD to drain at the end): it is used from ~40 work units per lane
            // (profiles/r02_ab_waves7.log; profiles/r02_wg_per_cu.log: 6 / 7 workgroups per CU = 78.2 / 76.1 ms for the bench frame, 39.8 / 38.8 for
            // half of it, 20.75 / 20.40 for a quarter, 10.95 / 10.95 for an eighth, 7.07 / 7.11 for C2).
            // (a large-workgroup build holds 24 waves per CU in its two workgroups: the rule never applies to it)
            if (wg_per_cu > 6u && (uint64_t)a.total_work < 40ull * c->n_cu * RTW_BLOCK * wg_per_cu) wg_per_cu = 6u;
        }
        uint32_t grid = (uint32_t)c->n_cu * wg_per_cu;
        {
            const uint32_t need = (a.total_work + block - 1) / block;
            if (grid > need) grid = need ? need : 1;
        }
        // Guided unit length (RTW_OPT_TAIL_UNITS = k; 0, the default, = one length for the whole launch).  The idea: the end of a
        // launch is one work unit deep per lane, so cut the LAST tiles of the queue into units of one sample and the tiles before them into units of
        // a third of the launch's length -- region 3 holds k blocks of (tile, 1 sample) for every resident wave, region 2 k blocks of (tile, L2
        // samples).  The image cannot change: the bank is indexed by (tile, sample, pixel) and the resolve adds in sample order.
        // MEASURED (profiles/r03_tail_units.log, r03_endtimes.log, r03_tail_order.log): it does what it says -- a wave runs on for 0.31 instead of
        // 0.40 ms on average after it finds the queue empty -- and gains nothing: an eighth of the bench frame 10.21 / 10.24 / 10.34 / 10.36 ms for
        // k = 0 / 1 / 2 / 4, C2 7.07 / 7.09 / 7.00 / 7.13, the whole frame 74.48 / 74.64 / 74.71 / 74.66.  What a launch waits for at its end is not
        // a unit but a PATH: with one-sample units the longest wait is still ~1.1 ms -- a 50-bounce glass path started just before the queue ran
        // dry, at ~20 us per segment with seven busy waves per SIMD -- and a path cannot be split.  Handing the sky tiles out last so that no such
        // path starts late (RTW_OPT_TILE_ORDER 5) does not help either.  Kept as an option; off.
        if (!sums && c->opt_tail_units > 0.0 && a.chunk_len > 1u && a.n_tiles > 1u) {
            const double waves = (double)grid * (block / 64u);
            const uint32_t L1 = a.chunk_len, L2 = L1 >= 12u ? 4u : (L1 >= 6u ? 2u : 1u), L3 = 1u;
            uint64_t t3 = (uint64_t)std::ceil(c->opt_tail_units * waves * L3 / (double)a.n_samples);
            uint64_t t2 = L2 > L3 ? (uint64_t)std::ceil(c->opt_tail_units * waves * L2 / (double)a.n_samples) : 0;
            if (t3 > a.n_tiles / 4u) t3 = a.n_tiles / 4u;                     // (small launches: at most a quarter of the tiles in either region)
            if (t2 > a.n_tiles / 4u) t2 = a.n_tiles / 4u;
            a.reg_q2 = a.n_tiles - (uint32_t)t3; a.reg_q1 = a.reg_q2 - (uint32_t)t2;
            a.reg_len[1] = L2; a.reg_len[2] = L3;
            for (int r = 1; r < 3; r++) a.reg_nc[r] = (a.n_samples + a.reg_len[r] - 1u) / a.reg_len[r];
            a.total_work = (a.reg_q1 * a.reg_nc[0] + (a.reg_q2 - a.reg_q1) * a.reg_nc[1] + (a.n_tiles - a.reg_q2) * a.reg_nc[2]) * 64u;   // <= tiles x samples x 64 < 2^32
        }
        {   // guided grabs (fetch_pixel): work left / (4 x resident waves), as a shift; at most RTW_OPT_GRAB_BLOCKS blocks (0: the blocks of one tile)
            a.sub_shift = (c->opt_sub_queues != 1u && a.n_tiles >= 64u && grid >= 64u) ? RTW_SUB_SHIFT : 0u;       // one sub-queue per XCD, unless the launch is tiny
            const uint32_t waves4 = (grid * (block / 64u) * 4u) >> a.sub_shift;
            a.grab_shift = 0; while (a.grab_shift < 31u && (1u << a.grab_shift) < waves4) a.grab_shift++;
            uint32_t blocks = c->opt_grab_blocks ? c->opt_grab_blocks : a.n_chunks;
            if (blocks > a.n_chunks) blocks = a.n_chunks;
            a.grab_max = (blocks ? blocks : 1u) * 64u;
        }
        HIP_TRY(hipMemsetAsync(a.queue, 0, RTW_QUEUE_BYTES, c->stream));
        if (a.n_tiles) { launch_render(fn, block, a, grid, c->stream); c->last_build = build; c->has_last_build = true; c->last_node_format = lds.node_format; }
        HIP_TRY(hipGetLastError());
        if (a.n_tiles) plans.push_back(queue_plan(a, grid, block));
        if (tile_rows == 0) break;
    }
    for (RtwQueuePlan &q : plans) q.bands = (uint32_t)plans.size();
    c->last_plans.swap(plans);
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipMemcpyAsync(c->scr.h_stats.ptr, a.stats, RTW_N_STATS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    c->pend.active = true; c->pend.n_rows = n_rows;
    c->pend.dst = out.base; c->pend.scatter = out.scatter; c->pend.direct = direct; c->pend.staged = staged;
    c->pend.width = p->width; c->pend.height = p->height; c->pend.row_block = a.row_block; c->pend.part_index = p->part_index; c->pend.part_count = p->part_count;
    c->pend.out_bytes = out_bytes;
    c->pend.enqueue_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - c->pend.t0).count();
    if (phases & PH_COPY) return render_copy(c);
    return RTW_OK;
}

// COPY phase: the rendered rows toward the caller's memory, queued behind the kernels on the context's stream.
static int render_copy(rtw_ctx *c) {
    if (!c || !c->pend.active) return RTW_E_INVALID;
    const rtw_ctx::Pending &q = c->pend;
    if (q.direct) return RTW_OK;                        // the kernels wrote into the caller's device buffer
    HIP_TRY(hipSetDevice(c->device));
    if (q.staged) {                                     // pinned staging now (a true asynchronous copy), the caller's pageable frame in render_wait
        HIP_TRY(hipMemcpyAsync(c->scr.h_out.ptr, c->scr.out.ptr, q.out_bytes, hipMemcpyDeviceToHost, c->stream));
    } else if (q.scatter) {
        const int rc = scatter_rows(c, c->scr.out.as<float>(), q.dst, q.width, q.height, q.row_block, q.part_index, q.part_count);
        if (rc != RTW_OK) return rc;
    } else HIP_TRY(hipMemcpyAsync(q.dst, c->scr.out.ptr, q.out_bytes, hipMemcpyDefault, c->stream));
    return RTW_OK;
}

// Wait for the render launched by render_enqueue and report its counters.
static int render_wait(rtw_ctx *c, RtwStats *stats) {
    if (!c || !c->pend.active) return RTW_E_INVALID;
    c->pend.active = false; c->pend.marked = false;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->pend.staged)
        scatter_rows_host(c->scr.h_out.as<float>(), c->pend.dst, c->pend.width, c->pend.height, c->pend.n_rows, c->pend.row_block, c->pend.part_index, c->pend.part_count);
    float ms = 0.0f, start_ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    HIP_TRY(hipEventElapsedTime(&start_ms, c->ev_mark, c->ev0));
    const unsigned long long *h_stats = c->scr.h_stats.as<unsigned long long>();
    const bool kernel_gave_up = h_stats[23] != 0ull;           // safety valve of the persistent loop (rtw_kernels.hip RTW_MAX_TRIPS)
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->camera_rays = h_stats[0]; stats->segments = h_stats[1];
        stats->sphere_tests = h_stats[2]; stats->node_tests = h_stats[3];
        stats->nan_pixels = (uint32_t)h_stats[4]; stats->rows = c->pend.n_rows;
        stats->quad_tests = h_stats[14];
        stats->kernel_ms = ms;
        stats->enqueue_ms = c->pend.enqueue_ms; stats->start_ms = start_ms;
        for (int k = 0; k < 3; k++) { stats->phase_steps[k] = h_stats[5 + k]; stats->phase_lanes[k] = h_stats[8 + k]; }
        for (int k = 3; k < 5; k++) { stats->phase_steps[k] = h_stats[16 + 2 * (k - 3)]; stats->phase_lanes[k] = h_stats[17 + 2 * (k - 3)]; }
#ifdef RTW_CENSUS                                   // diagnostic build only (scripts/gpu_census.py): lanes live in the sub-blocks of a SHADE step
        if (getenv("RTW_CENSUS_DUMP")) {
            static const char *names[CEN_N] = { "shading", "inflight (unit(d))", "miss (sky)", "hit (point, normal, material)", "dielectric branch", "schlick draw",
                                                "diffuse branch", "unit-vector loop trip", "bank store", "needs a work unit", "start_path", "lens-disk loop trip",
                                                "trav_begin", "depth exhausted", "trips through the scheduler (all phases)", "cooperative round" };
            std::fprintf(stderr, "rtw census: %llu SHADE steps\n", h_stats[7]);
            for (int k = 0; k < CEN_N; k++)
                if (h_stats[32 + 2 * k])
                    std::fprintf(stderr, "rtw census: %-32s executions %12llu (%.3f per SHADE step)  lanes %14llu  live fraction %.4f  lanes per SHADE step %.2f\n", names[k],
                                 h_stats[32 + 2 * k], (double)h_stats[32 + 2 * k] / (double)h_stats[7], h_stats[33 + 2 * k],
                                 (double)h_stats[33 + 2 * k] / (64.0 * (double)h_stats[32 + 2 * k]), (double)h_stats[33 + 2 * k] / (double)h_stats[7]);
        }
#endif
#if defined(RTW_STAMP) || defined(RTW_ENDTIMES)     // diagnostic builds only (scripts/gpu_endtimes.py)
        if (getenv("RTW_STAMP_DUMP")) std::fprintf(stderr, "rtw stamp: wave-ticks traverse %llu leaf %llu shade %llu   of shade (specialised builds): a. unit(d) + paths that end %llu, b. bank + next unit %llu, c-d. hit / path start + the rejection loop + second halves %llu, e. query begin %llu   (generic build: hit, bank + next unit, camera ray, query begin)\n",
                                                   h_stats[11], h_stats[12], h_stats[13], h_stats[16], h_stats[17], h_stats[18], h_stats[19]);
        if (getenv("RTW_ENDTIMES_DUMP") && h_stats[15] && getenv("RTW_ENDTIMES_REF")) {
            std::fprintf(stderr, "rtw endtimes histogram (waves ending in each 1/32 of the reference lifetime, bins 21/32 .. 32/32+; bin 0 also holds everything earlier):");
            for (int k = 0; k < 12; k++) std::fprintf(stderr, " %llu", h_stats[20 + k]);
            std::fprintf(stderr, "\n");
        }
        if (getenv("RTW_ENDTIMES_DUMP") && h_stats[15])
            std::fprintf(stderr, "rtw endtimes (100 MHz device clock): wave starts spread over %.1f us, first wave end %.1f us and last wave end %.1f us after the first start\n",
                         (double)(h_stats[25] - h_stats[24]) / 100.0, (double)(h_stats[26] - h_stats[24]) / 100.0, (double)(h_stats[27] - h_stats[24]) / 100.0);
        if (getenv("RTW_ENDTIMES_DUMP") && h_stats[15])
            std::fprintf(stderr, "rtw endtimes: the queue ran dry for the first wave %.1f us and for the last wave %.1f us after the first start; a wave then ran on for %.1f us on average, %.1f us at most\n",
                         (double)(h_stats[28] - h_stats[24]) / 100.0, (double)(h_stats[29] - h_stats[24]) / 100.0, (double)h_stats[31] / (double)h_stats[15] / 100.0, (double)h_stats[30] / 100.0);
        if (getenv("RTW_ENDTIMES_DUMP") && h_stats[15]) {   // RTW_ENDTIMES build: [12] longest wave lifetime [13] sum of wave lifetimes [15] waves
            if (h_stats[40]) {
                const double n = (double)h_stats[40];
                std::fprintf(stderr, "rtw endtimes: %llu waves ran on for 0.6 ms or more after finding the queue empty: on average %.0f us, %.0f scheduler trips (%.0f TRAVERSE steps with %.1f lanes, %.0f LEAF with %.1f, %.0f SHADE with %.1f), the busiest lane shaded %.1f queries, all lanes %.1f -> %.1f us per trip, %.1f us per query of the busiest lane\n",
                             h_stats[40], h_stats[41] / n / 100.0, h_stats[42] / n, h_stats[43] / n, h_stats[43] ? (double)h_stats[46] / h_stats[43] : 0.0, h_stats[44] / n, h_stats[44] ? (double)h_stats[47] / h_stats[44] : 0.0,
                             h_stats[45] / n, h_stats[45] ? (double)h_stats[48] / h_stats[45] : 0.0, h_stats[49] / n, h_stats[50] / n,
                             h_stats[42] ? h_stats[41] / 100.0 / h_stats[42] : 0.0, h_stats[49] ? h_stats[41] / 100.0 / h_stats[49] : 0.0);
            }
            std::fprintf(stderr, "rtw endtimes: %llu waves, longest lifetime %llu ticks, mean lifetime %.1f %% of it\n", h_stats[15], h_stats[12],
                         100.0 * (double)h_stats[13] / (double)h_stats[15] / (double)h_stats[12]);
        }
#endif
        stats->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - c->pend.t0).count();
    }
    return kernel_gave_up ? RTW_E_INTERNAL : RTW_OK;
}

struct rtw_mgpu {
    std::vector<rtw_ctx *> ctx;
};

extern "C" {

// A build printed in template order.
static int print_build(const RenderBuild &b, char *buf, size_t n) {
    const int len = b.bvh ? std::snprintf(buf, n, "render_bvh<%d,%d,%d,%d>", (int)b.moving, b.nodes, b.spec, (int)b.geom)
                          : std::snprintf(buf, n, "render_brute<%d,%d,%d>", (int)b.moving, b.spec, (int)b.geom);
    return len > 0 && (size_t)len < n ? RTW_OK : RTW_E_INVALID;
}

// Host only: the build the last launch ran.
int rtw_ctx_last_render_build(rtw_ctx *c, char *buf, size_t n) {
    if (!c || !buf || n == 0 || !c->has_last_build) return RTW_E_INVALID;
    return print_build(c->last_build, buf, n);
}

// Host only: render_enqueue_impl's three steps on the caller's facts.
int rtw_render_choice(const RtwRenderFacts *f, const RtwTreeFacts *t, int32_t opt_lds_geom, uint32_t opt_node_format, uint32_t moving, uint32_t accel,
                      RtwRenderChoice *out) {
    if (!f || !t || !out || accel > RTW_ACCEL_BVH || opt_lds_geom < -1 || opt_lds_geom > 1 || opt_node_format > 2u) return RTW_E_INVALID;
    const RenderChoice choice = render_choice(*f, *t, opt_lds_geom, opt_node_format, moving != 0u, accel == RTW_ACCEL_BVH);
    if (!choice.fn) return RTW_E_UNSUPPORTED;
    const LdsLayout &lds = choice.lds;
    *out = RtwRenderChoice{ {}, lds.node_format, lds.block, lds.stack_off, lds.geom_off, lds.tri_off, lds.bytes };
    return print_build(choice.build, out->build, sizeof out->build);
}

// Host only: the LDS node format the last launch's kernel read.
int rtw_ctx_last_node_format(rtw_ctx *c) {
    if (!c || !c->has_last_build) return RTW_E_INVALID;
    return (int)c->last_node_format;
}

// Host only: the work queue of band `band` of the last render, as launched.
int rtw_ctx_last_queue_plan(rtw_ctx *c, uint32_t band, RtwQueuePlan *out) {
    if (!c || !out || band >= c->last_plans.size()) return RTW_E_INVALID;
    *out = c->last_plans[band];
    return RTW_OK;
}

uint32_t rtw_mesh_list_max_default(void) { return RTW_MESH_LIST_MAX_DEFAULT; }

int rtw_ctx_set_option(rtw_ctx *c, uint32_t key, double v) {
    if (!c || !(v == v)) return RTW_E_INVALID;
    switch (key) {
    case RTW_OPT_CHUNK_LEN:      if (!(v >= 0.0 && v <= 255.0)) return RTW_E_INVALID; c->opt_chunk_len = (uint32_t)v; return RTW_OK;
    case RTW_OPT_SAMPLE_BANK_GB: if (!(v > 0.0 && v <= 1048576.0)) return RTW_E_INVALID; c->opt_bank_bytes = (uint64_t)(v * (double)(1ull << 30)); return RTW_OK;
    case RTW_OPT_LDS_GEOM:       if (!(v >= -1.0 && v <= 1.0)) return RTW_E_INVALID; c->opt_lds_geom = (int)v; return RTW_OK;
    case RTW_OPT_BLOCKS_PER_CU:  if (!(v >= 0.0 && v <= 8.0)) return RTW_E_INVALID; c->opt_blocks_per_cu = (uint32_t)v; return RTW_OK;
    case RTW_OPT_LIST_WALK_MAX:  if (!(v >= 0.0 && v <= 4294967295.0)) return RTW_E_INVALID; c->opt_list_walk_max = (uint32_t)v; return RTW_OK;
    case RTW_OPT_TILE_ORDER:     if (!(v >= 0.0 && v <= 5.0 && v == (double)(uint32_t)v)) return RTW_E_INVALID; c->opt_tile_order = (uint32_t)v; return RTW_OK;
    case RTW_OPT_SUB_QUEUES:     if (!(v == 0.0 || v == 1.0)) return RTW_E_INVALID; c->opt_sub_queues = (uint32_t)v; return RTW_OK;
    case RTW_OPT_TAIL_UNITS:     if (!(v >= 0.0 && v <= 1024.0)) return RTW_E_INVALID; c->opt_tail_units = v; return RTW_OK;
    case RTW_OPT_GUIDED_LAYOUT:  if (!(v >= 0.0 && v <= 4.0 && v == (double)(uint32_t)v)) return RTW_E_INVALID; c->opt_guided_layout = (uint32_t)v; return RTW_OK;
    case RTW_OPT_ATROUS_LAYOUT:  if (!(v == 0.0 || v == 1.0 || v == 2.0)) return RTW_E_INVALID; c->opt_atrous_layout = (uint32_t)v; return RTW_OK;
    case RTW_OPT_HISTOGRAM_COUNT: if (!(v == 0.0 || v == 1.0 || v == 2.0 || v == 3.0)) return RTW_E_INVALID; c->opt_histogram_count = (uint32_t)v; return RTW_OK;
    case RTW_OPT_GRAB_BLOCKS:    if (!(v >= 0.0 && v <= 65536.0 && v == (double)(uint32_t)v)) return RTW_E_INVALID; c->opt_grab_blocks = (uint32_t)v; return RTW_OK;
    case RTW_OPT_MESH_LIST_MAX:  if (!(v >= 0.0 && v <= 4294967295.0 && v == (double)(uint32_t)v)) return RTW_E_INVALID; c->opt_mesh_list_max = (uint32_t)v; return RTW_OK;
    case RTW_OPT_MESH_CLIMB:     if (!(v == 0.0 || v == 1.0 || v == 2.0)) return RTW_E_INVALID; c->opt_mesh_climb = (uint32_t)v; return RTW_OK;
    case RTW_OPT_NODE_FORMAT:    if (!(v == 0.0 || v == 1.0 || v == 2.0)) return RTW_E_INVALID; c->opt_node_format = (uint32_t)v; return RTW_OK;
    default: return RTW_E_INVALID;
    }
}

int rtw_ctx_render(rtw_ctx *c, const RtwCamera *cam, const RtwParams *p, float *out_rgb, RtwStats *stats) {
    int rc = render_enqueue(c, cam, p, OutSpec{ out_rgb, false });
    if (rc != RTW_OK) return rc;
    return render_wait(c, stats);
}

// ---- one frame over several GPUs (rtw.h) -------------------------------------------------------------
int rtw_mgpu_create(const int *devices, uint32_t n, rtw_mgpu **out) {
    if (!out) return RTW_E_INVALID;
    *out = nullptr;
    if (!devices || n == 0 || n > 64) return RTW_E_INVALID;
    if (rtw_device_count() <= 0) return RTW_E_NO_DEVICE;
    rtw_mgpu *m = new (std::nothrow) rtw_mgpu();
    if (!m) return RTW_E_NOMEM;
    for (uint32_t k = 0; k < n; k++) {
        rtw_ctx *c = nullptr;
        int rc = rtw_ctx_create(devices[k], &c);
        if (rc != RTW_OK) { rtw_mgpu_destroy(m); return rc; }
        m->ctx.push_back(c);
    }
    // let every device write into the others' memory (frames that live in one GPU's HBM); failure is fine: the copies then go
    // through the host, which hipMemcpyDefault does by itself
    for (uint32_t k = 0; k < n; k++) for (uint32_t j = 0; j < n; j++) {
        if (devices[k] == devices[j]) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, devices[k], devices[j]) == hipSuccess && can) {
            (void)hipSetDevice(devices[k]);
            if (hipDeviceEnablePeerAccess(devices[j], 0) != hipSuccess) (void)hipGetLastError();   // (already enabled is an error code too)
        } else (void)hipGetLastError();
    }
    *out = m;
    return RTW_OK;
}

void rtw_mgpu_destroy(rtw_mgpu *m) {
    if (!m) return;
    for (rtw_ctx *c : m->ctx) rtw_ctx_destroy(c);
    delete m;
}

int rtw_mgpu_set_scene(rtw_mgpu *m, const RtwScene *scene, float t_begin, float t_end) {
    if (!m) return RTW_E_INVALID;
    for (rtw_ctx *c : m->ctx) { int rc = rtw_ctx_set_scene(c, scene, t_begin, t_end); if (rc != RTW_OK) return rc; }
    return RTW_OK;
}

int rtw_mgpu_set_texture_noise(rtw_mgpu *m, const RtwPerlin *tables, uint32_t n_tables, const RtwTextureNoise *per_texture, uint32_t n_textures) {
    if (!m) return RTW_E_INVALID;
    for (rtw_ctx *c : m->ctx) { int rc = rtw_ctx_set_texture_noise(c, tables, n_tables, per_texture, n_textures); if (rc != RTW_OK) return rc; }
    return RTW_OK;
}

int rtw_mgpu_set_lights(rtw_mgpu *m, const RtwLight *lights, uint32_t n, float biased_weight) {
    if (!m) return RTW_E_INVALID;
    for (rtw_ctx *c : m->ctx) { int rc = rtw_ctx_set_lights(c, lights, n, biased_weight); if (rc != RTW_OK) return rc; }
    return RTW_OK;
}

int rtw_mgpu_set_instance_rotations(rtw_mgpu *m, const float (*qs)[4], uint32_t n) {
    if (!m) return RTW_E_INVALID;
    // every context holds the same scene: the list is checked against each before any context is touched, so a refusal leaves all as they were
    for (rtw_ctx *c : m->ctx) {
        if (!c->has_scene) return RTW_E_NO_SCENE;
        if (c->pend.active) return RTW_E_INVALID;
        if (qs || n) { const int rc = quats_check(c->h_instances.data(), (uint32_t)c->h_instances.size(), qs, n, nullptr); if (rc != RTW_OK) return rc; }
    }
    for (rtw_ctx *c : m->ctx) { int rc = rtw_ctx_set_instance_rotations(c, qs, n); if (rc != RTW_OK) return rc; }
    return RTW_OK;
}

int rtw_mgpu_set_triangles(rtw_mgpu *m, const RtwTriangle *tris, uint32_t n) {
    if (!m) return RTW_E_INVALID;
    for (rtw_ctx *c : m->ctx) { int rc = rtw_ctx_set_triangles(c, tris, n); if (rc != RTW_OK) return rc; }
    return RTW_OK;
}

int rtw_mgpu_set_mesh_instances(rtw_mgpu *m, const RtwMeshInstance *p, uint32_t n) {
    if (!m) return RTW_E_INVALID;
    // every context holds the same triangles: the list is checked against each before any context is touched, so a refusal leaves all as they were
    for (rtw_ctx *c : m->ctx) {
        if (!c->tris.n) return RTW_E_NO_SCENE;
        if (c->pend.active || (n && !p) || (!n && p) || n > RTW_MAX_MESH_INSTANCES) return RTW_E_INVALID;
        if (n && (c->tri_textured || !mesh_rows(p, n, nullptr))) return RTW_E_INVALID;
    }
    for (rtw_ctx *c : m->ctx) { int rc = rtw_ctx_set_mesh_instances(c, p, n); if (rc != RTW_OK) return rc; }
    return RTW_OK;
}

int rtw_mgpu_set_option(rtw_mgpu *m, uint32_t key, double value) {
    if (!m) return RTW_E_INVALID;
    for (rtw_ctx *c : m->ctx) { int rc = rtw_ctx_set_option(c, key, value); if (rc != RTW_OK) return rc; }
    return RTW_OK;
}

int rtw_mgpu_render(rtw_mgpu *m, const RtwCamera *cam, const RtwParams *params, float *out_rgb, RtwStats *per_device, RtwStats *total) {
    if (!m || !cam || !params || !out_rgb || params->part_count > 1) return RTW_E_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t n = (uint32_t)m->ctx.size();
    // fork: viewport.rs:236-240 spawns one task per row; here one asynchronous launch sequence per device, in three passes so that nothing
    // one device needs -- a first-use allocation, a driver query, a copy toward the caller's frame -- can delay the start of another:
    //   0. every device: mark the begin of the call on its stream, check the arguments, allocate what this frame shape needs (may wait)
    //   1. every device: memsets, kernels, events, counter read-back (never waits)
    //   2. every device: its rows toward the frame -- strided copies into device or pinned memory, pinned staging for a pageable frame
    int rc = RTW_OK;
    auto part = [&](uint32_t k) { RtwParams q = *params; q.row_block = params->row_block ? params->row_block : 8u; q.part_index = k; q.part_count = n; return q; };
    for (uint32_t k = 0; k < n && rc == RTW_OK; k++) {
        rtw_ctx *c = m->ctx[k];
        if (c->pend.active) { rc = RTW_E_INVALID; break; }
        c->pend.t0 = t0;
        if (hipSetDevice(c->device) != hipSuccess || hipEventRecord(c->ev_mark, c->stream) != hipSuccess) { (void)hipGetLastError(); rc = RTW_E_HIP; break; }
        c->pend.marked = true;
        const RtwParams q = part(k);
        rc = render_enqueue(c, cam, &q, OutSpec{ out_rgb, true }, PH_PREPARE);
    }
    uint32_t launched = 0;
    for (; launched < n && rc == RTW_OK; launched++) {
        const RtwParams q = part(launched);
        rc = render_enqueue(m->ctx[launched], cam, &q, OutSpec{ out_rgb, true }, PH_PREPARE | PH_LAUNCH);
        if (rc != RTW_OK) break;
    }
    for (uint32_t k = 0; k < launched && rc == RTW_OK; k++) rc = render_copy(m->ctx[k]);
    for (uint32_t k = 0; k < n; k++) m->ctx[k]->pend.marked = m->ctx[k]->pend.active && m->ctx[k]->pend.marked;
    // join: viewport.rs:241-244 awaits the tasks in order
    RtwStats sum; std::memset(&sum, 0, sizeof sum);
    for (uint32_t k = 0; k < launched; k++) {
        RtwStats st;
        const int rw = render_wait(m->ctx[k], &st);
        if (rw != RTW_OK) { if (rc == RTW_OK) rc = rw; continue; }
        if (per_device) per_device[k] = st;
        sum.camera_rays += st.camera_rays; sum.segments += st.segments; sum.sphere_tests += st.sphere_tests;
        sum.node_tests += st.node_tests; sum.quad_tests += st.quad_tests; sum.nan_pixels += st.nan_pixels; sum.rows += st.rows;
        for (int i = 0; i < 6; i++) { sum.phase_steps[i] += st.phase_steps[i]; sum.phase_lanes[i] += st.phase_lanes[i]; }
        if (st.kernel_ms > sum.kernel_ms) sum.kernel_ms = st.kernel_ms;
        if (st.enqueue_ms > sum.enqueue_ms) sum.enqueue_ms = st.enqueue_ms;          // (the last device's: the fork's length on the host)
        if (st.start_ms > sum.start_ms) sum.start_ms = st.start_ms;                // (the latest kernel start)
    }
    sum.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (total) *total = sum;
    return rc;
}

int rtw_render_multi_gpu(const int *devices, uint32_t n_devices, const RtwCamera *cam, const RtwScene *scene,
                         const RtwParams *params, float *out_rgb, RtwStats *per_device) {
    if (!cam || !scene || !params) return RTW_E_INVALID;
    rtw_mgpu *m = nullptr;
    int rc = rtw_mgpu_create(devices, n_devices, &m);
    if (rc != RTW_OK) return rc;
    rc = rtw_mgpu_set_scene(m, scene, cam->time0, cam->time0 + cam->shutter);
    if (rc == RTW_OK) rc = rtw_mgpu_render(m, cam, params, out_rgb, per_device, nullptr);
    rtw_mgpu_destroy(m);
    return rc;
}

int rtw_ctx_render_multi(rtw_ctx *c, const RtwCamera *cam, const RtwParams *p, float fps, uint32_t start_frame, uint32_t n_frames,
                         float *out_rgb, RtwStats *stats) {
    if (!c || !cam || !p || !out_rgb || !(fps > 0.0f)) return RTW_E_INVALID;
    const size_t frame_floats = (size_t)rtw_part_rows(p->height, p->row_block, p->part_index, p->part_count) * p->width * 3;
    for (uint32_t i = 0; i < n_frames; i++) {                     // viewport.rs:256-266, one async_render per frame
        RtwCamera cm = *cam;
        cm.time0 = host_div((float)(start_frame + i), fps);       // viewport.rs:279  frame as f32 / fps
        int rc = rtw_ctx_render(c, &cm, p, out_rgb + (size_t)i * frame_floats, stats ? stats + i : nullptr);
        if (rc != RTW_OK) return rc;
    }
    return RTW_OK;
}

int rtw_render(const RtwCamera *cam, const RtwScene *scene, const RtwParams *params, float *out_rgb, RtwStats *stats) {
    if (!cam || !scene || !params) return RTW_E_INVALID;
    int dev = 0;
    if (rtw_device_count() <= 0) return RTW_E_NO_DEVICE;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    rtw_ctx *c = nullptr;
    int rc = rtw_ctx_create(dev, &c);
    if (rc != RTW_OK) return rc;
    rc = rtw_ctx_set_scene(c, scene, cam->time0, cam->time0 + cam->shutter);
    if (rc == RTW_OK) rc = rtw_ctx_render(c, cam, params, out_rgb, stats);
    rtw_ctx_destroy(c);
    return rc;
}

} // extern "C"
