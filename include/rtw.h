/*
 * rtw.h -- C ABI of the MI355X-native path tracer (librtw_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of Terence-23/RayTracing-in-a-weekend:
 *
 *     Viewport::render / render_row  ->  ray_color_*  ->  Sphere::collision_normal  ->  Material::on_hit
 *
 * The reference has no FFI: its seam is the function-typed `ray_color` parameter of
 *   Rust/src/viewport.rs:430      Viewport::render(&self, ray_color: &dyn Fn(Ray,&Scene,usize)->Rgb<f32>, scene)
 *   Rust/src/viewport.rs:215-219  async_render(viewport: Box<Viewport>, ray_color, scene: Box<Scene>) -> Img
 *   Rust2/src/viewport.rs:116,128 Viewport::render_rows_async(self) / render(self)
 *   C++/headers/viewport.h:95     Img Viewport::Render(RGB_float (*ray_color)(...), const Scene&)
 * A host closure cannot cross to the GPU, so the integrator is selected by enum and the scene is
 * passed as flat PODs.  Everything here is plain C: pointers, sizes, PODs; no torch, no C++ types.
 *
 * Conventions
 *   - caller owns every buffer; the library allocates only device scratch inside an rtw_ctx
 *   - no exceptions / panics cross the ABI: 0 == RTW_OK, negative == RTW_E_*
 *   - rtw_ctx_render() is blocking (mirrors `rt.block_on(render_multi(..))`, Rust/src/main.rs:76-78)
 *   - one rtw_ctx == one GPU == one HIP stream; contexts are independent (one per process/rank)
 *   - all arithmetic is f32 (Rust/src/vec3.rs:11-15)
 */
#ifndef RTW_H
#define RTW_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTW_ABI_VERSION 4

/* ---- status codes ------------------------------------------------------------------------- */
#define RTW_OK              0
#define RTW_E_INVALID      -1   /* bad argument (NULL pointer, zero size, unknown enum value)        */
#define RTW_E_NO_DEVICE    -2   /* no HIP device / device index out of range                         */
#define RTW_E_HIP          -3   /* a HIP runtime call failed (rtw_last_hip_error() has the code)     */
#define RTW_E_NOMEM        -4   /* host or device allocation failed                                  */
#define RTW_E_UNSUPPORTED  -5   /* valid enum value that this build does not implement on the device */
#define RTW_E_NO_SCENE     -6   /* rtw_ctx_render() before rtw_ctx_set_scene()                       */
#define RTW_E_INTERNAL     -7   /* a render kernel gave up (safety valve of its persistent loop): the image is incomplete */
#define RTW_E_RUNTIME_CONFLICT -8 /* rtw_ctx_create: two copies of the HIP runtime are loaded in this process (PyTorch imported after the
                                     first rtw_* call): import torch first, see INTEGRATION.md.  v4 */

/* ---- integrators: which `ray_color` closure the reference would have passed ----------------- */
enum {
    RTW_INTEGRATOR_GRADIENT = 0, /* ray_color_gradient, Rust/src/viewport/ray_color.rs:12-41 (== ray_color_d main.rs:17-46) */
    RTW_INTEGRATOR_BG_COLOR = 1, /* ray_color_bg_color, Rust/src/viewport/ray_color.rs:43-92 (emission + background)        */
    RTW_INTEGRATOR_NORMAL   = 2, /* normal shading of the closest hit, C++/src/tests.cpp:76-97 (ray_colorSc)                */
    RTW_INTEGRATOR_FLAG     = 3, /* RNG-free yellow/blue test integrator, Rust/src/viewport/glass_tests.rs:8-54             */
    RTW_INTEGRATOR_RUST2    = 4, /* Rust2 `ray_color` (Rust2/src/viewport/ray_color.rs:12-37): emmited + next * multiplied,
                                    depth 0 and misses return the background, with Rust2's Material trait objects
                                    (Rust2/src/objects/material.rs): opacity > 0 -> MirrorGlass{ir}, metallicness == 1 ->
                                    Mirror (reflects the UN-normalised direction), else Lambertian (unit(n + rand));
                                    with RTW_FLAG_MIXED_MATERIAL opacity < 0 -> MixedMaterial{exp = ir};
                                    ColorResult{emmited, multiplied} = {emitted, tex * col_mod}                             */
    RTW_INTEGRATOR_LIGHT_CAST = 5,   /* Rust2 `light_biased_ray_cast` (Rust2/src/viewport/ray_color.rs:55-108): ONE surface hit and a shadow ray
                                    towards every light of rtw_ctx_set_lights; RtwParams.depth is ignored; a miss returns the background */
    RTW_INTEGRATOR_LIGHT_BIASED = 6  /* Rust2 `light_biased_ray_color` (ray_color.rs:111-164): RTW_INTEGRATOR_RUST2's path, draw for draw,
                                    plus one shadow ray per light at every surface hit (see "light-biased integrators" below)       */
};

/* ---- samplers: which driver loop generates the camera rays ---------------------------------- */
enum {
    RTW_SAMPLER_ROW        = 0, /* render_row: exactly `samples` unstratified, shutter time; Rust/src/viewport.rs:270-305 */
    RTW_SAMPLER_STRATIFIED = 1, /* Viewport::render: ceil(sqrt(samples))^2 strata, time 0; Rust/src/viewport.rs:430-478   */
    RTW_SAMPLER_CENTRES    = 2, /* Rust2 render_row: floor(sqrt(samples))^2 fixed centres; Rust2/src/viewport.rs:87-114   */
    RTW_SAMPLER_NO_RAND    = 3  /* render_no_rand: one un-jittered ray per pixel; Rust/src/viewport.rs:479-516            */
};

/* ---- closest-hit strategy (result-invariant) ------------------------------------------------ */
enum {
    RTW_ACCEL_BRUTE = 0, /* every sphere, list order (the reference's test integrators: camera_tests.rs:19-33)   */
    RTW_ACCEL_BVH   = 1  /* device BVH, time-expanded bounds (Scene::collision_normal -> AABB, viewport.rs:136-150) */
};

/* ---- PODs ----------------------------------------------------------------------------------- */

/* The render-time fields of `Viewport` (Rust/src/viewport.rs:49-77), produced by
 * rtw_viewport_new() == Viewport::new (viewport.rs:308-401).  `pixel00` is
 * `upper_left_corner`: a DIRECTION (the origin is not added, viewport.rs:377-378). */
typedef struct RtwCamera {
    float origin[3];
    float u[3];
    float v[3];
    float pixel00[3];
    float delta_u[3];     /* p_delta_u */
    float delta_v[3];     /* p_delta_v */
    float lens_radius;
    float time0;          /* frame as f32 / fps            (viewport.rs:279) */
    float shutter;        /* shutter_speed                 (viewport.rs:297) */
} RtwCamera;

/* `Sphere` (Rust/src/objects/sphere.rs:13-20) with its `Material` (materials.rs:15-20) inlined.
 * `tex < 0` means the sphere carries the 1x1 ImageTexture::from_color(tex_color) that
 * Sphere::new builds (sphere.rs:151-173); the albedo the hit reports is texel * col_mod
 * (sphere.rs:145), so Sphere::new(c) yields c*c -- that quirk is reproduced by passing
 * tex_color == col_mod == c. */
typedef struct RtwSphere {
    float center[3];      /* origin                                   */
    float radius;
    float velocity[3];    /* centre(t) = origin + velocity * ray.time  (sphere.rs:100) */
    float col_mod[3];
    float tex_color[3];
    float metallicness;
    float opacity;        /* > 0 selects the dielectric branch (materials.rs:106) */
    float ir;
    float emitted[3];     /* `emmited` */
    int32_t tex;          /* index into RtwScene.textures, or -1 */
} RtwSphere;

/* `ImageTexture{img,row,col}` (Rust/src/texture.rs:21-27): row == width, col == height,
 * texel (x,y) lives at texels[3*(texel_offset + y*row + x)] (texture.rs:265).  The texture's optional Perlin noise
 * (`ImageTexture.noise` / `noise_scale`) is set per context with rtw_ctx_set_texture_noise (RtwTextureNoise, below). */
typedef struct RtwTexture {
    uint32_t row;
    uint32_t col;
    uint32_t texel_offset;
    uint32_t emit_tex;    /* RTW_INTEGRATOR_RUST2 only: 1 + index of the texture that holds Rust2's `emmit_img` for this image
                             (Rust2/src/objects/texture.rs:34-41), 0 = none (the sphere's `emitted` is used).  Was `reserved` (0) up to v3. */
} RtwTexture;

/* `Quad` (Rust/src/objects/quad.rs:8-20) with its `Material` inlined.  The derived fields of Quad::new
 * (normal = unit(u x v), d = normal . origin, w = n / n.n; quad.rs:96-108) are recomputed by the library.
 * A quad has no col_mod: the hit's albedo is the texel alone (quad.rs:64-79) -- tex < 0 means the 1x1
 * ImageTexture::from_color(tex_color), else texel (floor(alfa*row), floor(beta*col)) of textures[tex].
 * `velocity` is carried by the reference's struct but not used by its hit test (quad.rs:37-81). */
typedef struct RtwQuad {
    float origin[3];
    float u[3];
    float v[3];
    float velocity[3];
    float tex_color[3];
    float metallicness;
    float opacity;
    float ir;
    float emitted[3];
    int32_t tex;
} RtwQuad;

/* `Instance` (Rust/src/objects/instance.rs:27-38): a group of spheres and quads with a translation and an
 * Euler rotation (Vec3::rotated, vec3.rs:161-181 -- restated as written, including its non-orthogonal
 * terms for rotations about more than one axis), hit in local coordinates (instance.rs:250-310).
 * medium != 0 selects `dist_fn = const_density` (instance.rs:24-26): the hit becomes a scattering event
 * at distance ln(xi) / -density behind the surface with a random normal (constant-density smoke). */
enum { RTW_MEDIUM_SURFACE = 0, RTW_MEDIUM_CONST_DENSITY = 1 };
typedef struct RtwInstance {
    uint32_t first_sphere, n_spheres;   /* members: RtwScene.inst_spheres[first_sphere .. +n_spheres) */
    uint32_t first_quad, n_quads;       /*          RtwScene.inst_quads[first_quad .. +n_quads)       */
    float translation[3];
    float rotation[3];
    float density;
    uint32_t medium;                    /* RTW_MEDIUM_* */
} RtwInstance;

/* `Scene` (Rust/src/viewport.rs:79-151): spheres, quads, instances, background colour.  Sphere-only callers
 * (Scene::new_sphere) leave everything after `background` zero. */
typedef struct RtwScene {
    const RtwSphere  *spheres;
    const RtwTexture *textures;   /* may be NULL when n_textures == 0 */
    const float      *texels;     /* [n_texels][3], may be NULL       */
    uint32_t n_spheres;
    uint32_t n_textures;
    uint32_t n_texels;
    float    background[3];       /* Scene.background_color (BG_COLOR / RUST2 integrators) */
    const RtwQuad     *quads;         /* Scene.quads                                       */
    const RtwInstance *instances;     /* Scene.instances                                   */
    const RtwSphere   *inst_spheres;  /* member pools of the instances                     */
    const RtwQuad     *inst_quads;
    uint32_t n_quads;
    uint32_t n_instances;
    uint32_t n_inst_spheres;
    uint32_t n_inst_quads;
} RtwScene;

typedef struct RtwParams {
    uint32_t width, height;       /* full image; each at most 65535 (RTW_E_INVALID beyond) */
    uint32_t samples;             /* Viewport.samples (see sampler for the count actually traced) */
    uint32_t depth;               /* Viewport.depth: max closest-hit queries per camera ray       */
    float    gamma;               /* output = powf(mean, 1/gamma) (viewport.rs:207-213)           */
    float    mint, maxt;          /* 0.001 / 1e5 in ray_color_gradient, 1e4 bg_color, 1e3 ray_color_d */
    uint32_t integrator;          /* RTW_INTEGRATOR_* */
    uint32_t sampler;             /* RTW_SAMPLER_*    */
    uint32_t accel;               /* RTW_ACCEL_*      */
    uint32_t flags;               /* RTW_FLAG_*       */
    uint64_t seed;                /* render seed of the counter-based RNG (DESIGN.md "RNG") */
    /* Row partition for multi-GPU: this call renders the rows r with
     *   (r / row_block) % part_count == part_index,
     * written compactly in increasing r to out_rgb[rows][width][3].
     * part_count <= 1 renders every row. */
    uint32_t row_block;
    uint32_t part_index;
    uint32_t part_count;
    uint32_t reserved;
} RtwParams;

#define RTW_FLAG_NONE            0u
#define RTW_FLAG_RECURSIVE_ORDER 1u  /* oracle only: multiply col_mod in the reference's recursion order */
#define RTW_FLAG_CPP_DIELECTRIC  2u  /* the C++ twin's deterministic dielectric (Schlick term commented out,
                                        C++/headers/materials.h:106): refract whenever possible, no draw */
#define RTW_FLAG_GLOBAL_NODES    4u  /* device only: keep the BVH nodes in global memory (f32, 64 B) even when the
                                        f16 LDS-resident copy is available -- for A/B measurements and tests */
#define RTW_FLAG_CPP_DIFFUSE     8u  /* the C++ twin's non-dielectric branch (C++/headers/materials.h:113-117,
                                        C++/src/materials.cpp:4-13, C++/src/vec3.cpp:28-39, C++/src/sphere.cpp:29-31), in f32:
                                        rejection accepts |p|^2 < 1 (not <= 1); the diffuse direction is
                                        unit((point + normal + rand_unit) - point); the mirror direction is normalised again,
                                        unit(reflect(unit(d), n)); a near-zero (1e-8) result becomes the normal.
                                        RTW_FLAG_CPP_DIELECTRIC | RTW_FLAG_CPP_DIFFUSE is what Viewport::RenderGPU of the C++
                                        tree asks for. */
#define RTW_FLAG_CHUNK_SUMS     16u  /* keep ONE partial sum per pixel and RTW_SUM_CHUNK consecutive samples in the device's sample bank instead
                                        of every sample: the samples of a chunk are added left to right, the chunks' sums in chunk order,
                                        ((s0+s1+s2+s3) + (s4+..)) + ..  Deterministic and independent of the GPU split like the default, but
                                        not the reference's left-to-right association (viewport.rs:299): the image differs by f32 rounding
                                        only (<= 2e-6 relative, far inside BASELINE.json's 1e-3).  The bank shrinks 4x (12.4 GB -> 3.1 GB at
                                        1920x1080x500).  The oracle implements the same association under the same flag. */
#define RTW_SUM_CHUNK            4u
#define RTW_FLAG_MIXED_MATERIAL 32u  /* Rust2's MixedMaterial (see "MixedMaterial" below): under RTW_INTEGRATOR_RUST2 / _LIGHT_CAST / _LIGHT_BIASED an
                                        object with opacity < 0 is MixedMaterial::new(ir), a Phong lobe of exponent ir about the normal.  With any
                                        other integrator: RTW_E_UNSUPPORTED.  Without the flag opacity < 0 selects what it always did. */

typedef struct RtwStats {
    uint64_t camera_rays;    /* (pixel, sample) primary rays traced                   */
    uint64_t segments;       /* closest-hit queries == BASELINE "rays x bounces"      */
    uint64_t sphere_tests;   /* exact ray/sphere quadratic evaluations                */
    uint64_t node_tests;     /* BVH node slab tests (0 for RTW_ACCEL_BRUTE); with triangles also the triangle-tree node visits */
    uint32_t nan_pixels;     /* output pixels with a NaN channel                      */
    uint32_t rows;           /* rows written by this call                             */
    float    kernel_ms;      /* device time of the render kernels (hipEvent)          */
    float    total_ms;       /* host wall time of the call                            */
    /* BVH kernel scheduler census: wave-level steps executed per phase (0 traverse, 1 leaf, 2 shade; 3..5 reserved for
     * experimental phases) and the lanes that were live in them; lanes / (64 * steps) is the SIMD efficiency of a phase. */
    uint64_t phase_steps[6];
    uint64_t phase_lanes[6];
    uint64_t quad_tests;     /* ray/quad plane tests (top-level quads and instance members) and ray/triangle plane tests */
    /* v4: the call's timeline.  enqueue_ms: host time from the begin of the call (rtw_mgpu_render: of the whole call, the same instant for
     * every device) until this context's kernels had been issued; start_ms: device time from a marker recorded on this context's stream at
     * the begin of the call (before any device was given work) to the start of its first kernel.  A fork that is asynchronous shows
     * enqueue_ms far below kernel_ms for EVERY device, and on distinct GPUs start_ms near zero for every device. */
    float    enqueue_ms;
    float    start_ms;
} RtwStats;

typedef struct rtw_ctx rtw_ctx;

/* ---- device path (librtw_hip.so) ------------------------------------------------------------ */

int         rtw_abi_version(void);
int         rtw_device_count(void);
const char *rtw_strerror(int status);
int         rtw_last_hip_error(void);
int         rtw_hip_runtime_count(void);   /* copies of libamdhip64 mapped into this process (1 is healthy; v4) */

/* One context per GPU.  `device` is the HIP device ordinal. */
int  rtw_ctx_create(int device, rtw_ctx **out);
void rtw_ctx_destroy(rtw_ctx *ctx);
/* Launch on this HIP stream (a hipStream_t passed as void*): every copy, kernel and event of every later rtw_ctx_* call is enqueued on
 * it, so the call is ordered behind the work the caller enqueued there before it, and each call still returns only when its own work
 * is done.  NULL = the context's own stream.  That stream is created hipStreamNonBlocking: it orders with NO other stream, the
 * default stream included, so whatever produces a device buffer handed to a call on it must have finished before the call.
 * The handle 0 is therefore NOT the default stream (which PyTorch calls its default stream and hands out as cuda_stream == 0): name
 * that one with RTW_STREAM_LEGACY, HIP's hipStreamLegacy.  Any other non-NULL handle is passed to HIP as it is; the caller keeps the
 * stream alive while it is set. */
#define RTW_STREAM_LEGACY ((void *)1)
int  rtw_ctx_set_stream(rtw_ctx *ctx, void *hip_stream);
/* == Scene::new_sphere(spheres) (viewport.rs:90-105): copies the scene to the GPU and builds the
 * acceleration structure.  [t_begin, t_end] is the ray.time range the bounds must cover
 * (time0 .. time0 + shutter); pass 0,0 for static scenes.  The range is remembered: a later render of a
 * MOVING scene whose [time0, time0 + shutter] is not inside it walks the list instead of the tree (same image,
 * slower) rather than pruning with bounds that do not cover the spheres. */
int  rtw_ctx_set_scene(rtw_ctx *ctx, const RtwScene *scene, float t_begin, float t_end);
/* == Viewport::render(ray_color, scene) -> Img.  out_rgb is [rows][width][3] f32, gamma-corrected,
 * unclamped (viewport.rs:301); it may be host memory or device memory of ctx's GPU. */
int  rtw_ctx_render(rtw_ctx *ctx, const RtwCamera *cam, const RtwParams *params,
                    float *out_rgb, RtwStats *stats);
/* == render_multi(viewport, ray_color, scene) -> Vec<Img> (Rust/src/viewport.rs:249-269): frames start_frame .. start_frame +
 * n_frames, frame i rendered like async_render with time0 = i as f32 / fps (viewport.rs:279; cam->time0 is ignored, cam->shutter
 * is the shutter_speed).  out_rgb holds n_frames images of [rows][width][3] f32 back to back (host or device memory); stats, if not
 * NULL, is an array of n_frames.  The scene must have been set for the whole clip:
 * rtw_ctx_set_scene(ctx, scene, start_frame / fps, (start_frame + n_frames - 1) / fps + shutter). */
int  rtw_ctx_render_multi(rtw_ctx *ctx, const RtwCamera *cam, const RtwParams *params, float fps,
                          uint32_t start_frame, uint32_t n_frames, float *out_rgb, RtwStats *stats);
/* One-shot convenience: create ctx on the current device, set scene, render, destroy.  Renders without texture noise
 * (use a context and rtw_ctx_set_texture_noise for that). */
int  rtw_render(const RtwCamera *cam, const RtwScene *scene, const RtwParams *params,
                float *out_rgb, RtwStats *stats);

/* Tuning knobs of a context (they were process environment variables up to ABI v2).  None of them changes the image. */
enum {
    RTW_OPT_CHUNK_LEN        = 1, /* samples per work unit, 1..255; 0 = chosen from the size of the launch (default)           */
    RTW_OPT_SAMPLE_BANK_GB   = 2, /* budget of the per-sample radiance bank in GiB (default 48); larger frames are
                                     rendered in bands of tile rows, a budget below one tile row fails with RTW_E_NOMEM  */
    RTW_OPT_LDS_GEOM         = 3, /* sphere {centre, r^2} in LDS next to the f16 nodes: -1 auto (default), 0 off, 1 on   */
    RTW_OPT_BLOCKS_PER_CU    = 4, /* resident workgroups per CU of the persistent grid: 0 auto (default), 1..8           */
    RTW_OPT_LIST_WALK_MAX    = 5, /* RTW_ACCEL_BVH requests for scenes with at most this many spheres walk the list
                                     instead (result-invariant; the traversal scheduler only costs there).  Default:
                                     the measured crossover; 0 = always use the tree                     */
    RTW_OPT_TILE_ORDER       = 6, /* order in which the 8x8 tiles enter the work queue: 0 (default) raster; 1 groups of 8
                                     tiles scattered over the frame; 2 expensive tiles first by a cost estimated from each tile's centre
                                     ray (sphere field / ground only / sky, nearer first; raster for scenes with quads or instances);
                                     3 reverse raster; 4 as 2 in 32 coarse steps per class, raster inside a step; 5 raster inside each
                                     class, classes in the order sphere field, bare ground, sky (v4; measured: no gain)                    */
    RTW_OPT_GRAB_BLOCKS      = 7, /* 64-item blocks of the work queue a wave may take with one atomic while plenty of work is left (single
                                     blocks towards the end of a launch): default 2; 1 = always one; 0 = up to one tile's blocks      */
    RTW_OPT_TAIL_UNITS       = 9, /* guided unit length: the last tiles of the work queue are cut into units of ONE sample (k blocks of them per
                                     resident wave, k = this value) and the tiles before them into units of a third of the launch's length;
                                     0 (default) = one unit length for the whole launch.  Measured: no gain.  v4                 */
    RTW_OPT_SUB_QUEUES       = 8, /* 0 (default): the work queue is eight sub-queues with a counter each (a wave starts on the one of its
                                     XCD and helps out on the others when it is empty), a single one for tiny launches; 1: always single */
    RTW_OPT_GUIDED_LAYOUT    = 10,/* rtw_ctx_guided_filter: 0 (default) places the weight table and the guide tile by size;
                                     1 table and guides in LDS, 2 guides only, 3 table only, 4 neither -- followed where it fits in LDS  */
    RTW_OPT_NODE_FORMAT      = 11,/* how a static sphere scene's tree lives in LDS where the common-configuration builds of the BVH render
                                     kernel serve it: 0 (default) as f32 planes, walked by workgroups of 768 threads, where two of them fit a
                                     CU's LDS, else as f16 nodes; 1 f16 nodes (the build that keeps the sphere geometry in LDS too, whatever
                                     RTW_OPT_LDS_GEOM says); 2 f32 planes wherever one workgroup fits.  Other builds walk f16 nodes whatever
                                     it says.  Any other value: RTW_E_INVALID.  The walk, the counters and the image are the same */
    RTW_OPT_MESH_LIST_MAX    = 12,/* contexts with at most this many mesh placements meet them in list order even under RTW_ACCEL_BVH
                                     (result-invariant; the "mesh placements" section); more walk the top-level tree over the placements.
                                     Default RTW_MESH_LIST_MAX_DEFAULT, the measured crossover; 0 = always the top-level
                                     tree, 4294967295 = never; a value that is not a whole number: RTW_E_INVALID.  (added within v4)                                                         */
    RTW_OPT_MESH_CLIMB       = 13,/* how rtw_ctx_move_mesh_instances climbs the top-level tree: 0 (default) by the tree's node count, the
                                     measured choice; 1 one launch per height; 2 one launch of one workgroup.  The bytes are the
                                     same.  Any other value: RTW_E_INVALID.  (added within v4)                                              */
    RTW_OPT_ATROUS_LAYOUT    = 14,/* where a level of rtw_ctx_atrous_filter reads its taps: 0 (default) the measured choice per level
                                     (DESIGN.md 8c); 1 from an LDS tile of the workgroup's pixels and their halo wherever that tile fits; 2 from
                                     global memory.  The bytes are the same.  Any other value: RTW_E_INVALID.  (added within v4)
                                     rtw_ctx_svgf_filter's levels and rtw_ctx_variance_estimate's window follow it too, and
                                     so do rtw_ctx_colour_bounds' window (8h) and rtw_ctx_upsample_filter's low window (8i), and every
                                     step of rtw_ctx_bloom (8k: 0 = the measured choice per kernel and level size).                       */
    RTW_OPT_HISTOGRAM_COUNT  = 15,/* how a workgroup of rtw_ctx_luminance_histogram keeps its LDS counts: 0 (default) the measured choice
                                     (DESIGN.md 8j); 1 one LDS histogram, one LDS atomic a pixel; 2 one LDS histogram a wave, summed at the
                                     end; 3 one LDS histogram, the lanes of a wave that share the first active lane's slot added as one
                                     atomic.  The counts are the same.  Any other value: RTW_E_INVALID.  (added within v4)              */
};
int  rtw_ctx_set_option(rtw_ctx *ctx, uint32_t key, double value);
/* Which compiled build of the render kernel the context's last render launched, as text in template-argument order:
 * "render_brute<MOVING,SPEC,GEOM>" or "render_bvh<MOVING,NODES,SPEC,GEOM>", e.g. "render_bvh<1,2,5,0>" (every band of one render runs the
 * same build).  Host only: no device work.  RTW_E_INVALID before the context's first render, or when the n bytes of buf are too few (32 are
 * enough).  For tests and diagnostics: which build serves a request is not part of the contract.  (added within v4) */
int  rtw_ctx_last_render_build(rtw_ctx *ctx, char *buf, size_t n);
/* ... and the format of the tree that build read from LDS: 0 none (list walk, or nodes in global memory), 1 f16 nodes, 2 f32 planes
 * (RTW_OPT_NODE_FORMAT).  Host only.  RTW_E_INVALID before the context's first render.  (added within v4) */
int  rtw_ctx_last_node_format(rtw_ctx *ctx);
/* ... and the work queue that render handed to its kernel, one record per band of tile rows, as launched: the band's compact
 * rows [k_base, k_end) and tiles, the samples per pixel and how they are cut into units (chunk_len, n_chunks: the first region's; bank_len 1:
 * one bank slot per unit, RTW_FLAG_CHUNK_SUMS), the three regions of unit length over the queue positions [0, reg_q1), [reg_q1, reg_q2),
 * [reg_q2, n_tiles) with reg_len[r] samples per unit and reg_nc[r] units per pixel, total_work = 64 items per (tile, unit), 2^sub_shift
 * sub-queues, the guided grab (grab_shift, grab_max items), the grid and the threads per workgroup, whether a tile order was handed over
 * (0 / 1), and the row partition.  bands: how many bands the render had (the same in every record).  Host only: no device work; a copy of
 * what was launched, nothing is computed again.  RTW_E_INVALID for a NULL pointer, before the context's first render, and for
 * band >= bands; a render that is refused leaves the records of the last one that was launched.  For tests and diagnostics: how a render
 * is cut into work is not part of the contract.  (added within v4) */
typedef struct RtwQueuePlan {
    uint32_t bands, n_tiles, tiles_x, k_base, k_end;
    uint32_t n_samples, chunk_len, n_chunks, bank_len;
    uint32_t reg_q1, reg_q2, reg_len[3], reg_nc[3], total_work;
    uint32_t sub_shift, grab_shift, grab_max;
    uint32_t grid, block;
    uint32_t has_tile_order;
    uint32_t row_block, part_index, part_count;
} RtwQueuePlan;
int  rtw_ctx_last_queue_plan(rtw_ctx *ctx, uint32_t band, RtwQueuePlan *out);
/* Host only (no context, no GPU), for tests and diagnostics: the build and the dynamic LDS layout a render would launch, from plain facts
 * -- the same functions the render itself calls, once each.  RtwRenderFacts: what the request needs -- the integrator, sampler, depth and
 * flags of RtwParams (RTW_FLAG_MIXED_MATERIAL only where the scene holds a MixedMaterial object), whether a sphere has an image texture,
 * and counts (or 0 / 1) of quads, instances, textures with noise in use, triangles, instance rotations and mesh placements.  RtwTreeFacts:
 * the sphere tree as rtw_bvh_dump describes it (has_planes: 1 wherever has_f16 is), and the scene's sphere count.  opt_lds_geom /
 * opt_node_format: RTW_OPT_LDS_GEOM and RTW_OPT_NODE_FORMAT.  moving: a sphere moves.  accel: the strategy actually walked, i.e. after the
 * downgrades of a BVH request to the list walk (RTW_OPT_LIST_WALK_MAX, cameras and ranges the tree does not serve).  out->build is the
 * text rtw_ctx_last_render_build prints, node_format what rtw_ctx_last_node_format answers, block the threads per workgroup; the LDS
 * numbers are bytes (lds_geom_off 0: the sphere geometry stays in global memory; lds_tri_off: the triangle build's counter, the last 16 bytes of a
 * request with triangles).  RTW_E_INVALID on a null pointer or an accel / option out of range, RTW_E_UNSUPPORTED when no such build is compiled.
 * (added within v4) */
typedef struct RtwRenderFacts {
    uint32_t integrator, sampler, depth, flags, has_textures;
    uint32_t n_quads, n_instances, noise, n_triangles, rotations, placements;
} RtwRenderFacts;
typedef struct RtwTreeFacts { uint32_t n_nodes, depth, n_spheres, has_f16, has_planes; } RtwTreeFacts;
typedef struct RtwRenderChoice {
    char build[32];
    uint32_t node_format, block, lds_stack_off, lds_geom_off, lds_tri_off, lds_bytes;
} RtwRenderChoice;
int  rtw_render_choice(const RtwRenderFacts *request, const RtwTreeFacts *tree, int32_t opt_lds_geom, uint32_t opt_node_format,
                       uint32_t moving, uint32_t accel, RtwRenderChoice *out);

/* ---- one frame over several GPUs of a node ------------------------------------------------------
 * The reference forks one task per image row and joins them in order (tokio: Rust/src/viewport.rs:236-244; rayon:
 * Rust2/src/viewport.rs:119-122).  Here the rows are dealt to the devices in interleaved blocks of `row_block` rows
 * (RtwParams.row_block, 8 when 0; device k renders the rows r with (r / row_block) % n_devices == k) and every device
 * copies its blocks STRAIGHT INTO their image rows of the caller's frame (one strided 2-D copy per device, no gather
 * buffer, no de-interleave pass).  The counter-based RNG makes the image independent of the split: the result is bit-identical
 * to rtw_ctx_render of the whole frame on one GPU.  One host thread drives all devices; the call blocks until the frame is
 * complete.  The fork is asynchronous by construction: first every device is prepared (arguments, first-use allocations), then
 * every device's kernels are issued, and only then the copies toward the caller's frame -- none of which waits for a GPU: a frame
 * in device memory or in pinned host memory (hipHostMalloc / hipHostRegister) receives the strided copies directly, a frame in
 * ordinary pageable host memory (where a device-to-host copy would return only when it is done) is staged through a pinned buffer
 * per device and finished by the host at the join.  RtwStats.enqueue_ms / start_ms of per_device[] show the timeline.
 * `devices` are HIP ordinals and may repeat (several contexts on one GPU).  NOT YET MEASURED on more than one physical GPU.
 * out_rgb: the full [height][width][3] f32 frame, host memory or device memory of any of the GPUs.
 * params->part_count must be <= 1.  per_device (may be NULL): n_devices RtwStats; total (may be NULL): counters summed,
 * kernel_ms = the slowest device, total_ms = host wall time of the call. */
typedef struct rtw_mgpu rtw_mgpu;
int  rtw_mgpu_create(const int *devices, uint32_t n_devices, rtw_mgpu **out);
void rtw_mgpu_destroy(rtw_mgpu *m);
int  rtw_mgpu_set_scene(rtw_mgpu *m, const RtwScene *scene, float t_begin, float t_end);
int  rtw_mgpu_set_option(rtw_mgpu *m, uint32_t key, double value);
int  rtw_mgpu_render(rtw_mgpu *m, const RtwCamera *cam, const RtwParams *params, float *out_rgb,
                     RtwStats *per_device, RtwStats *total);
/* One-shot: create, set scene for [cam->time0, cam->time0 + cam->shutter], render, destroy.  Renders without texture noise. */
int  rtw_render_multi_gpu(const int *devices, uint32_t n_devices, const RtwCamera *cam, const RtwScene *scene,
                          const RtwParams *params, float *out_rgb, RtwStats *per_device);

/* ---- Perlin noise of image textures (Rust/src/texture.rs:61-194, 259-267) ----------------------------------------------------
 * `ImageTexture{noise: Option<PerlinNoise>, noise_scale}`: every texel the texture returns is multiplied by noise(p / noise_scale), p the
 * hit point (spheres: r.at(t) in world space, also for a moving sphere; quads: the hit point; members of an instance: the point in the
 * instance's LOCAL frame; constant-density media: the local point of the boundary hit).  The 1x1 textures of Sphere::new / Quad::new
 * (tex < 0) never carry noise.  A scale of 0 is not rejected: p / 0 is inf or NaN and flows through as in the reference. */
typedef struct RtwPerlin {            /* PerlinNoise (texture.rs:61-68); ranfloat is never read by noise(), so it is not carried */
    float   ranvec[256][3];
    uint8_t perm_x[256], perm_y[256], perm_z[256];
} RtwPerlin;
typedef struct RtwTextureNoise {      /* per RtwTexture: ImageTexture.noise / noise_scale */
    int32_t perlin;                   /* index into the table array, -1 = no noise */
    float   scale;
} RtwTextureNoise;
/* PerlinNoise::new (texture.rs:110-149) from `seed`: ranvec[i] = Vec3::random(-1, 1).unit() with the scene generators' PCG32 (the
 * reference draws from the OS: its tables cannot be reproduced).  The permutations are the identity, as the reference's
 * create_permute leaves them (its shuffle loop runs over the empty range 255..0).  Host only. */
int rtw_perlin_new(uint64_t seed, RtwPerlin *out);
/* PerlinNoise::noise (turb_depth == 0) or PerlinNoise::turb(p, turb_depth) at n points [n][3] on the host: out[n]. */
int rtw_perlin_eval(const RtwPerlin *t, const float *points, uint32_t n, uint32_t turb_depth, float *out);
/* The same on ctx's GPU (the function the render kernels call), host buffers in and out; blocking. */
int rtw_ctx_perlin_eval(rtw_ctx *ctx, const RtwPerlin *t, const float *points, uint32_t n, uint32_t turb_depth, float *out);
/* Noise of the textures of the scene of the last rtw_ctx_set_scene (which clears it): per_texture[i] for RtwScene.textures[i],
 * n_textures == the scene's texture count, every perlin index < n_tables (or -1).  per_texture == NULL with n_textures == 0 clears it.
 * RTW_E_NO_SCENE before any scene.  While a texture that a sphere, quad or instance member uses has noise, renders run the noise build
 * of the generic kernel, and RTW_INTEGRATOR_RUST2 (whose textures have no noise) fails with RTW_E_UNSUPPORTED.  The tables are copied. */
int rtw_ctx_set_texture_noise(rtw_ctx *ctx, const RtwPerlin *tables, uint32_t n_tables,
                              const RtwTextureNoise *per_texture, uint32_t n_textures);
/* The same on every device of m (rtw_mgpu_set_scene clears it). */
int rtw_mgpu_set_texture_noise(rtw_mgpu *m, const RtwPerlin *tables, uint32_t n_tables,
                               const RtwTextureNoise *per_texture, uint32_t n_textures);

/* ---- bilateral filter of a frame (Rust2/src/postprocessing.rs:12-131) -----------------------------------------------------------
 * `bilateral_filter(img, Proximity::new(size, Square | Edges))`, the post-process Rust2 runs on the 8-bit image of render_rows_async
 * (postprocessing.rs:444-447), reproduced bit for bit: spatial = ceil(0.02 sqrt(w*w + h*h)); the range term is the mean of the
 * intensity gradient over the interior pixels, summed serially in the reference's order (rows outer, columns inner); the window of a
 * pixel is x - min(x, size) .. x + min(w-x-1, size) by y - min(y, size) .. y + min(h-y-1, size), both half-open (the neighbours at +size
 * are never taken), column outer, row inner; Edges keeps the taps with |dx| + |dy| < size.  Every weight is libm expf of an argument
 * that depends only on (dx*dx + dy*dy, |channel difference|): the library tabulates them on the host and the device looks them up.
 * The output byte is `(col_sum * 255 / w_sum) as u8` (truncated, saturated, NaN -> 0): a uniform image (mean gradient 0) and size 0
 * come out all zeros, as in the reference.
 * img / out are [h][w][3], row-major; w >= 3, h >= 3 (the reference's (w-2)*(h-2) underflows below), w*w + h*h must fit in u32, and
 * size <= RTW_BILATERAL_MAX_SIZE (the window holds (2 size)^2 taps; larger sizes return RTW_E_INVALID). */
#define RTW_BILATERAL_MAX_SIZE 64u
enum { RTW_PROXIMITY_SQUARE = 0, RTW_PROXIMITY_EDGES = 1 };          /* ProximityType (postprocessing.rs:12-15) */
enum { RTW_PIXELS_U8 = 0,                                            /* [h][w][3] uint8_t                                           */
       RTW_PIXELS_F32_RUST2 = 1 };                                   /* [h][w][3] float, quantised first as rtw_quantize_u8_rust2 */
typedef struct RtwBilateral {
    uint32_t size;                  /* Proximity.size, 0 .. RTW_BILATERAL_MAX_SIZE                                   */
    uint32_t proximity;             /* RTW_PROXIMITY_SQUARE | RTW_PROXIMITY_EDGES                                    */
    uint32_t in_format;             /* RTW_PIXELS_U8 | RTW_PIXELS_F32_RUST2                                          */
    float    avg_gradient;          /* 0 = computed as the reference does; > 0 (finite) = used as given, the gradient pass is skipped */
} RtwBilateral;
typedef struct RtwFilterStats {
    float    avg_gradient;          /* the range term used (computed or given)                                      */
    float    spatial;               /* ceil(0.02 sqrt(w*w + h*h))                                                    */
    float    gradient_ms;           /* device: the gradient terms and their serial sum (0 when skipped); host: the serial sum */
    float    table_ms;              /* host time to build the weight table (and, on the device path, to enqueue its upload) */
    float    filter_ms;             /* device: the filter kernel (hipEvent); host: the per-pixel loop                 */
    float    total_ms;              /* host wall time of the call                                                    */
    uint64_t taps;                  /* window entries evaluated over the whole image (each is 3 weights)             */
} RtwFilterStats;
/* The host form (the library's CPU path, the same table and serial sum; threads over rows). */
int rtw_bilateral_filter(const void *in, uint32_t w, uint32_t h, const RtwBilateral *params, uint8_t *out, RtwFilterStats *stats);
/* On ctx's GPU, on its stream, blocking.  `in` and `out` may be host memory or device memory of ctx's GPU.  Needs no scene and leaves
 * the scene, and every render, untouched.  stats may be NULL. */
int rtw_ctx_bilateral_filter(rtw_ctx *ctx, const void *in, uint32_t w, uint32_t h, const RtwBilateral *params, uint8_t *out,
                             RtwFilterStats *stats);

/* ---- guided (joint / cross bilateral) filter: the bilateral filter steered by depth, normal and object-id buffers ----------------------
 * rtw_bilateral_filter with every tap's three channel weights multiplied by one guide weight g, formed from the buffers that
 * rtw_ctx_depth_map / rtw_ctx_scene_hits write.  For centre pixel p and tap q, in f32, one rounding per written operation:
 *     a = 0
 *     if sigma_depth  > 0:  dz = depth[q] - depth[p];   a = a + inv_depth  * (dz * dz)
 *     if sigma_normal > 0:  d  = normal[q] - normal[p]; a = a + inv_normal * ((d.x*d.x + d.y*d.y) + d.z*d.z)
 *     g = (a >= 0) ? exp_plain(-a) : 0                  (a NaN a -- inf - inf, a NaN depth -- drops the tap)
 *     if same_object and idx[q] != idx[p]:  g = 0
 *     w_c = table[d2][|k_c|] * g;   col_sum[c] += (q[c] * w_c) / 255;   w_sum[c] += w_c
 * with inv_depth = 0.5f / (sigma_depth * sigma_depth), inv_normal likewise, and exp_plain the library's own exponential (rtw_exp_plain:
 * the same bits on the host and on the GPU).  Everything else -- formats, spatial, the range term or a given avg_gradient, the window
 * with its half-open quirk, the tap order, Edges, the libm weight table, the output byte -- is rtw_bilateral_filter's.  With no term on, g
 * is not applied and the output is rtw_bilateral_filter's bit for bit; so it is with guides that are constant over the image (g = 1).
 * Guides: depth [h][w] f32, normal [h][w][3] f32, idx [h][w] i32, row-major.  A miss of rtw_ctx_depth_map (depth maxt * 1.6, normal 0 0 0,
 * idx -1) is simply another depth, normal and object.  A guide whose term is off may be NULL and is never read.
 * RTW_E_INVALID: everything rtw_bilateral_filter refuses; a sigma that is negative or not finite, or so small that its inv_* is not finite;
 * sigma_depth > 0 with depth == NULL; sigma_normal > 0 with normal == NULL; same_object with idx == NULL; same_object > 1.
 * There is no rtw_mgpu_* form and no JSON form. */
typedef struct RtwGuidedFilter {
    RtwBilateral base;              /* size, proximity, in_format, avg_gradient: as rtw_bilateral_filter             */
    float    sigma_depth;           /* 0 = no depth term; else in the units of `depth`                               */
    float    sigma_normal;          /* 0 = no normal term; else in units of |n - n'|                                 */
    uint32_t same_object;           /* 1 = a tap on another idx weighs 0                                             */
} RtwGuidedFilter;
/* The host form (threads over rows).  RtwFilterStats as rtw_bilateral_filter: taps counts window entries. */
int rtw_guided_filter(const void *in, uint32_t w, uint32_t h, const float *depth, const float *normal, const int32_t *idx,
                      const RtwGuidedFilter *params, uint8_t *out, RtwFilterStats *stats);
/* On ctx's GPU, on its stream, blocking; the bytes of the host form.  `in`, `out` and each guide may independently be host memory or
 * device memory of ctx's GPU (host memory is staged).  Needs no scene and leaves the scene, and every render, untouched. */
int rtw_ctx_guided_filter(rtw_ctx *ctx, const void *in, uint32_t w, uint32_t h, const float *depth, const float *normal,
                          const int32_t *idx, const RtwGuidedFilter *params, uint8_t *out, RtwFilterStats *stats);

/* ---- a-trous filter: an edge-avoiding wavelet filter of linear f32 frames (Dammertz et al. 2010) -- added within v4 -------------------
 * Multi-scale where the two filters above have one scale, on the linear frame where they work on its 8-bit quantisation, and steered by
 * the same guide buffers (depth [h][w] f32, normal [h][w][3] f32, idx [h][w] i32: what rtw_ctx_depth_map / rtw_ctx_scene_hits write).  With
 * `albedo` (and `emitted`) it filters (rgb - emitted) / albedo, so that texture is kept.  in, out, albedo, emitted are [h][w][3] f32,
 * row-major.  Everything is f32 with one rounding per written operation (no fused multiply-add), exp_plain is rtw_exp_plain's:
 *   demodulate:  a_c = (albedo && albedo[p][c] >= albedo_floor) ? albedo[p][c] : 1;  e_c = emitted ? emitted[p][c] : 0;
 *                C0[p][c] = (in[p][c] - e_c) / a_c
 *   level i = 0 .. levels-1, step s = 1 << i: the taps q = p + s * (dx, dy), dy = -2..2 outer, dx = -2..2 inner, those outside the frame
 *   skipped;  hw = K[|dx|] * K[|dy|], K = {3/8, 1/4, 1/16};  a = 0
 *     if sigma_color  > 0:  d = Ci[q] - Ci[p];                  a = a + inv_color_i * ((d.x*d.x + d.y*d.y) + d.z*d.z)
 *     if sigma_depth  > 0:  dz = (depth[q] - depth[p]) * 2^-i;  a = a + inv_depth * (dz * dz)
 *     if sigma_normal > 0:  d = normal[q] - normal[p];          a = a + inv_normal * ((d.x*d.x + d.y*d.y) + d.z*d.z)
 *     g = (a >= 0) ? exp_plain(-a) : 0;   if same_object and idx[q] != idx[p]:  g = 0;   wt = hw * g
 *     if wt > 0:  sum_c = sum_c + Ci[q][c] * wt;  wsum = wsum + wt
 *   Ci+1[p] = wsum > 0 ? sum / wsum : Ci[p]
 *   remodulate:  out[p][c] = C_levels[p][c] * a_c + e_c
 * with inv_x = 0.5f / (sigma_x * sigma_x) and inv_color_i formed from sigma_color * 2^-i.  A tap of weight 0 adds nothing: for finite
 * values that is the plain sum's bits, and with the colour term on it lets a NaN or infinite tap drop out (its a is NaN) while a NaN
 * centre keeps its own value (every a is NaN, wsum stays 0).  A miss of rtw_ctx_depth_map is simply another depth, normal and object.
 * `out` may be `in`.  A guide whose term is off, `albedo` and `emitted` may be NULL; an off guide is never read.
 * RTW_E_INVALID, nothing written: in, out or params NULL; w or h zero or beyond RTW_ATROUS_MAX_SIDE, or w * h beyond 32 bits; levels
 * outside 1 .. RTW_ATROUS_MAX_LEVELS; a sigma that is negative or not finite, or so small that its inv_* is not finite at some level;
 * sigma_depth > 0 with depth NULL, sigma_normal > 0 with normal NULL, same_object with idx NULL; same_object > 1; with albedo given, an
 * albedo_floor that is not finite or not > 0.  There is no rtw_mgpu_* form and no JSON form. */
#define RTW_ATROUS_MAX_LEVELS 8u
#define RTW_ATROUS_MAX_SIDE   0x7FFFFC00u   /* a pixel coordinate plus two steps of the last level stays a 32-bit integer */
typedef struct RtwAtrous {
    uint32_t levels;                /* 1 .. RTW_ATROUS_MAX_LEVELS; level i steps by 2^i pixels                        */
    float    sigma_color;           /* 0 = no colour term; level i uses sigma_color * 2^-i                           */
    float    sigma_depth;           /* 0 = no depth term; else in the units of `depth`                               */
    float    sigma_normal;          /* 0 = no normal term; else in units of |n - n'|                                 */
    uint32_t same_object;           /* 1 = a tap on another idx weighs 0                                             */
    float    albedo_floor;          /* used when albedo != NULL: a channel below it is not demodulated               */
} RtwAtrous;
/* The host form (one thread).  RtwFilterStats: filter_ms and total_ms are the call's time, taps counts the taps inside the frame over all
 * levels, the other fields are 0. */
int rtw_atrous_filter(const float *in, uint32_t w, uint32_t h, const float *depth, const float *normal, const int32_t *idx,
                      const float *albedo, const float *emitted, const RtwAtrous *params, float *out, RtwFilterStats *stats);
/* On ctx's GPU, on its stream, blocking; the bytes of the host form.  Every buffer may independently be host memory or device memory of
 * ctx's GPU (host memory is staged).  One launch per level over two buffers the context owns (RTW_OPT_ATROUS_LAYOUT); filter_ms is the
 * device time of all launches.  Needs no scene and leaves the scene, and every render, untouched. */
int rtw_ctx_atrous_filter(rtw_ctx *ctx, const float *in, uint32_t w, uint32_t h, const float *depth, const float *normal,
                          const int32_t *idx, const float *albedo, const float *emitted, const RtwAtrous *params, float *out,
                          RtwFilterStats *stats);

/* ---- temporal accumulation: frames of a sequence blended along reprojected pixels -- added within v4 ------------------------------------
 * The a-trous filter's temporal half (Schied et al. 2017, SVGF's accumulation): the previous call's accumulated colour, its two luminance
 * moments and its history length are fetched where each pixel's surface point lay in the previous view, accepted or rejected per tap
 * against the surface buffers, and blended with the new frame.  For cameras of rtw_viewport_new and the ray rule RTW_RAYS_PIXEL only; the
 * world is taken as static between the two frames (rtw_temporal_accumulate_motion, below, takes rigid motions of objects).  Everything is f32 with one rounding per written operation (no fused multiply-add); a
 * dot product is (x*x' + y*y') + z*z', a cross product x x y = (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0).
 * Buffers, row-major: cur, *_color, *_normal [h][w][3] f32; *_moments [h][w][2] f32; *_len, *_depth, *_variance [h][w] f32; *_idx [h][w]
 * i32.  depth, normal, idx are what rtw_ctx_surface_map(.., RTW_RAYS_PIXEL, offset, ..) writes for `cam`, prev_depth, prev_normal, prev_idx
 * what it wrote for prev_cam; a miss is simply another depth, normal and object.  prev_color, prev_moments, prev_len are the previous
 * call's out_color, out_moments, out_len.
 *   The plan, once per call on the host, from prev_cam (p00 = pixel00, du = delta_u, dv = delta_v):
 *     n = du x dv;  a = dv x n;  b = n x du;  pn = p00.n;  pa = p00.a;  pb = p00.b;  ua = du.a;  vb = dv.b
 *     static = cam and prev_cam agree byte for byte in origin, pixel00, delta_u, delta_v
 *   Pixel p = (i, j), (ox, oy) = params.offset:
 *     L = (0.2126f r + 0.7152f g) + 0.0722f b of cur[p];   fin = r, g, b all finite
 *     static:     fx = i;  fy = j;  s = depth[p]
 *     otherwise:  dir = the direction of rtw_pixel_rays for `cam` at (i, j) with the offset;  P = cam.origin + dir * depth[p];
 *                 d = P - prev_cam.origin;  s = (d.n) / pn;  fx = ((d.a) / s - pa) / ua - ox;  fy = ((d.b) / s - pb) / vb - oy
 *                 (s is the t the previous depth buffer holds for a ray through (fx, fy) that meets P)
 *     no history unless s > 0, fx > -1, fx < w, fy > -1, fy < h (all false for NaN)
 *     x0 = floorf(fx), wx = fx - x0, y likewise; the taps q, in this order: (x0, y0) with wt = (1-wx)*(1-wy), (x0+1, y0) with wx*(1-wy),
 *     (x0, y0+1) with (1-wx)*wy, (x0+1, y0+1) with wx*wy.  A tap counts when it lies inside the frame, prev_len[q] > 0,
 *         depth_tol  > 0:  |prev_depth[q] - s| <= depth_tol * s
 *         normal_cos > 0:  normal[p] . prev_normal[q] >= normal_cos
 *         same_object:     prev_idx[q] == idx[p]
 *     and wt > 0 (a tap of weight 0 adds nothing, as in the a-trous filter: it cannot enter as 0 * NaN).  Over the counted taps
 *         wsum = wsum + wt;  sum_x = sum_x + wt * prev_x[q]   for the 3 colour channels, the 2 moments and the length
 *     a history exists when wsum > 0: H = sum / wsum
 *     with a history and fin:   n_ = H.len + 1 < max_history ? H.len + 1 : max_history;  a_ = 1 / n_, alpha when a_ < alpha;  am_ likewise
 *                               with alpha_moments;  out_color = H.c + (cur - H.c) * a_;  m1 = H.m1 + (L - H.m1) * am_;
 *                               m2 = H.m2 + (L*L - H.m2) * am_;  out_len = n_
 *     no history, fin:          out_color = cur;  m1 = L;  m2 = L*L;  out_len = 1
 *     a history, not fin:       the history is written back unchanged, out_len = H.len: one bad sample does not enter
 *     no history, not fin:      out_color = cur;  m1 = m2 = 0;  out_len = 0: no later frame reads this pixel as history
 *     out_moments = (m1, m2);   out_variance = m2 - m1*m1 when that is > 0, else 0
 * The first frame passes NULL for prev_cam, prev_color, prev_moments, prev_len and the three prev_* guides: every pixel is without a
 * history.  A guide whose term is off may be NULL and is never read (depth is always read).  out_color may be cur: a pixel reads only its
 * own cur.  out_variance may be NULL.  History coverage is the caller's mean of out_len > 1.
 * RTW_E_INVALID, nothing written: cur, cam, depth, params, out_color, out_moments or out_len NULL; w or h zero or beyond
 * RTW_TEMPORAL_MAX_SIDE, or w * h beyond 32 bits; some but not all of prev_cam, prev_color, prev_moments, prev_len given, or a prev_* guide
 * without them; a term that is on with its current guide NULL, or, with a history, its previous guide NULL; alpha or alpha_moments outside
 * [0, 1] or not finite; max_history outside 1 .. 65535; depth_tol negative or not finite; normal_cos outside [0, 1] or not finite;
 * same_object > 1; an offset that is not finite; a prev_cam whose pn, ua or vb is zero or not finite; out_color == prev_color,
 * out_moments == prev_moments or out_len == prev_len (neighbours gather from prev_*).
 * There is no rtw_mgpu_* form and no JSON form. */
#define RTW_TEMPORAL_MAX_SIDE 65535u
typedef struct RtwTemporal {
    float    alpha;                 /* floor of the colour blend factor, 0 .. 1 (0: plain running mean up to max_history) */
    float    alpha_moments;         /* the same for the two luminance moments                                         */
    uint32_t max_history;           /* 1 .. 65535: history length saturates here                                      */
    float    depth_tol;             /* 0 = no depth test; else a tap passes when |prev_depth[q] - s| <= depth_tol * s */
    float    normal_cos;            /* 0 = no normal test; else in (0, 1]: normal[p] . prev_normal[q] >= normal_cos   */
    uint32_t same_object;           /* 1 = a tap passes only when prev_idx[q] == idx[p]                               */
    float    offset[2];             /* the RTW_RAYS_PIXEL offset both frames' guides were made with                   */
} RtwTemporal;
/* The host form (one thread).  RtwFilterStats: filter_ms and total_ms are the call's time, taps = 4 * w * h, the other fields are 0. */
int rtw_temporal_accumulate(const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth, const float *normal,
                            const int32_t *idx, const RtwCamera *prev_cam, const float *prev_color, const float *prev_moments,
                            const float *prev_len, const float *prev_depth, const float *prev_normal, const int32_t *prev_idx,
                            const RtwTemporal *params, float *out_color, float *out_moments, float *out_len,
                            float *out_variance /* may be NULL */, RtwFilterStats *stats);
/* On ctx's GPU, on its stream, blocking; the bytes of the host form.  Every buffer may independently be host memory or device memory of
 * ctx's GPU (host memory is staged; results go straight into device buffers).  One launch, one thread per pixel; filter_ms is its device
 * time.  Needs no scene and leaves the scene, and every render, untouched. */
int rtw_ctx_temporal_accumulate(rtw_ctx *ctx, const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth,
                                const float *normal, const int32_t *idx, const RtwCamera *prev_cam, const float *prev_color,
                                const float *prev_moments, const float *prev_len, const float *prev_depth, const float *prev_normal,
                                const int32_t *prev_idx, const RtwTemporal *params, float *out_color, float *out_moments, float *out_len,
                                float *out_variance /* may be NULL */, RtwFilterStats *stats);

/* ---- temporal accumulation with moving objects: one rigid motion per top-level object -- added within v4 ---------------------------------
 * rtw_temporal_accumulate takes the world as static between the two frames.  Here a table of rows says, per top-level object, where a world
 * point of the object lay in the previous frame; row k belongs to the object rtw_ctx_surface_map reports as idx first + k (mesh placement k
 * is n_spheres + n_quads + n_instances + k).  Everything of "temporal accumulation" above holds, f32 with one rounding per written
 * operation, but for a pixel that has a row:
 *   Which pixels have a row:  rows != NULL, and with k = idx[p] - first formed without wrap-around (in 64 bits): 0 <= k < n_rows and
 *     rows[k].moving != 0.  A miss (-1), an id below first, an id at or beyond first + n_rows and every other i32 value have no row, and no
 *     address is formed from them.
 *   Without a row:  the rule above, byte for byte, its per-call `static` shortcut included.
 *   With a row r:   dir and P = cam.origin + dir * depth[p] as in the rule's "otherwise" line, under a static camera too;
 *                   e = P - r.from;   P'_c = ((r.a[3c] e0 + r.a[3c+1] e1) + r.a[3c+2] e2) + r.to_c;   d = P' - prev_cam.origin;
 *                   s, fx, fy from d as above; the four taps as above (never the static shortcut's one tap); and the normal test reads
 *                   n'_c = (r.nrm[3c] n0 + r.nrm[3c+1] n1) + r.nrm[3c+2] n2  (n = normal[p])  in place of normal[p].
 *                   A NaN in a, from or to gives an s or fx that is NaN -- "no history" by the comparisons above, never an index; a NaN in
 *                   nrm fails the normal test when that is on.
 * Points and normals of a mesh placement turn by different matrices (a placement meets a ray turned by its quaternion and reports the
 * normal turned by the same quaternion, "mesh placements" below), so a row carries both; rtw_mesh_instance_motion makes such rows.
 * idx must be given when rows is given, whether or not same_object is on (prev_idx only for that term).
 * out_prev_xy [h][w][2] f32 (may be NULL) receives (fx, fy) as computed for every pixel of a call that has a history -- (i, j) under the
 * shortcut; also where the candidate box then rejects the pixel -- and (NaN, NaN) on a first frame.
 * RTW_E_INVALID, nothing written: the refusals above; rows with idx NULL; rows with n_rows == 0; first + n_rows beyond 2^31; out_prev_xy
 * equal to out_color, out_moments, out_len or out_variance.  With rows NULL, n_rows and first are not read.
 * With rows == NULL and out_prev_xy == NULL the calls write the bytes of rtw_temporal_accumulate / rtw_ctx_temporal_accumulate.
 * What stays out: the moving spheres of ray.time, a wider search when all four taps fail (deforming meshes: "temporal accumulation with
 * per-pixel motion", below).  There is no rtw_mgpu_* form and no JSON form. */
typedef struct RtwMotionRow {
    float    a[9];      /* row-major 3 x 3: world points, current frame -> previous frame        */
    float    from[3];   /* subtracted before a is applied (the object's current position)       */
    float    to[3];     /* added after (its previous position)                                  */
    float    nrm[9];    /* row-major 3 x 3: the normals surface_map writes, current -> previous */
    uint32_t moving;    /* 0: the object did not move; nothing else of the row is read          */
    uint32_t pad[7];
} RtwMotionRow;
/* The host form (one thread); stats as rtw_temporal_accumulate's. */
int rtw_temporal_accumulate_motion(const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth, const float *normal,
                                   const int32_t *idx, const RtwCamera *prev_cam, const float *prev_color, const float *prev_moments,
                                   const float *prev_len, const float *prev_depth, const float *prev_normal, const int32_t *prev_idx,
                                   const RtwTemporal *params, const RtwMotionRow *rows /* may be NULL */, uint32_t n_rows, uint32_t first,
                                   float *out_color, float *out_moments, float *out_len, float *out_variance /* may be NULL */,
                                   float *out_prev_xy /* may be NULL */, RtwFilterStats *stats);
/* On ctx's GPU, on its stream, blocking; the bytes of the host form.  rows and out_prev_xy, like every other buffer, may be host memory
 * (staged) or device memory of ctx's GPU.  One launch, one thread per pixel: with rows or out_prev_xy a second instantiation of the
 * kernel, chosen on the host; without them the launch of rtw_ctx_temporal_accumulate. */
int rtw_ctx_temporal_accumulate_motion(rtw_ctx *ctx, const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth,
                                       const float *normal, const int32_t *idx, const RtwCamera *prev_cam, const float *prev_color,
                                       const float *prev_moments, const float *prev_len, const float *prev_depth,
                                       const float *prev_normal, const int32_t *prev_idx, const RtwTemporal *params,
                                       const RtwMotionRow *rows /* may be NULL */, uint32_t n_rows, uint32_t first, float *out_color,
                                       float *out_moments, float *out_len, float *out_variance /* may be NULL */,
                                       float *out_prev_xy /* may be NULL */, RtwFilterStats *stats);

/* The rows of mesh placements that moved from prev_poses to cur_poses, both [n][7] f32 = position xyz, quaternion wxyz as
 * rtw_ctx_move_mesh_instances takes them; rows_out [n] RtwMotionRow.  With (qn_c, pos_c) and (qn_p, pos_p) the normalised quaternion
 * and position the walk uses for the two poses ("mesh placements" below), rotate(q, v) its rotation, e_j the unit vectors:
 *   column j of a   = rotate(conj(qn_p), rotate(qn_c, e_j))      (a ray meets the placement at conj(qn).rotate(x') + position)
 *   column j of nrm = rotate(qn_p, rotate(conj(qn_c), e_j))      (the reported normal is qn.rotate(n'))
 *   from = pos_c;  to = pos_p;  pad = 0;  conj is three exact negations
 *   moving = 0 exactly when the two poses agree in all 28 bytes; such a row is the identity (a = nrm = I, from = to = 0)
 *   else a pose the placements refuse on either side (a component that is not finite, a quaternion of length 0 or not finite) gives
 *   moving = 1, the quiet NaN 0x7fc00000 in all of a, from = to = 0 and the identity in nrm: its pixels have no history.
 * The call still returns RTW_OK; *n_invalid (may be NULL) counts the rows with a refused pose on either side, equal poses included (a
 * move leaves such a placement where it was).  RTW_E_INVALID: a NULL pointer, n == 0 or n > RTW_MAX_MESH_INSTANCES.  Host only, pure. */
int rtw_mesh_instance_motion(const float *prev_poses, const float *cur_poses, uint32_t n, RtwMotionRow *rows_out, uint32_t *n_invalid);
/* On ctx's GPU, on its stream, blocking; the bytes of the host form, one thread per placement.  Each of the three buffers may be host
 * memory (input staged, result copied back) or device memory of ctx's GPU (read and written in place).  Needs no scene. */
int rtw_ctx_mesh_instance_motion(rtw_ctx *ctx, const float *prev_poses, const float *cur_poses, uint32_t n, RtwMotionRow *rows_out,
                                 uint32_t *n_invalid);

/* ---- temporal accumulation with per-pixel motion: deforming meshes, and any geometry the caller moves itself -- added within v4 ------------
 * A row carries a rigid object.  A mesh that rtw_ctx_refit_triangles deforms has no such row: where a surface point lay a frame ago depends
 * on its triangle and its place inside it.  Three pieces close that gap, each f32 with one rounding per written operation, no fused
 * multiply-add, dot products as (x*x' + y*y') + z*z':
 *   1. rtw_ctx_surface_map_tri / rtw_ctx_scene_surface_tri ("surface buffers" below) report the triangle under each ray and (alfa, beta).
 *   2. rtw_deform_motion turns them, with the PREVIOUS frame's ouv rows, into each pixel's previous world point and the normal it had there:
 *        a pixel has a point when 0 <= tri[p] < n_tris (no wrap-around); {o, u, v} = row tri[p] of prev_ouv ([n_tris][9] as
 *        rtw_ctx_refit_triangles takes it; the caller kept it, the context does not hold the old mesh)
 *          x'_c = (o_c + alfa * u_c) + beta * v_c;     n' = unit(u x v) as Triangle::new forms it (n / |n|)
 *        prev_poses == NULL:  prev_point = x', carried_normal = n'  (idx, n_mesh and first are not read)
 *        else ([n_mesh][7] as rtw_ctx_move_mesh_instances took them a frame ago): k = idx[p] - first in 64 bits, 0 <= k < n_mesh or the
 *          pixel has no point; (qn, pos) the normalised quaternion and position the walk uses for pose k ("mesh placements" below):
 *          prev_point = rotate(conj(qn), x') + pos;   carried_normal = rotate(qn, n');   a pose the placements refuse: no point
 *        a pixel without a point: the quiet NaN 0x7fc00000 in all six floats; no address is formed from such a tri or k.
 *        A degenerate previous triangle (u x v = 0) gives a finite point and a normal that is not finite: it fails the normal test when
 *        that is on, and only then.
 *      RTW_E_INVALID, nothing written: a NULL tri, bary, prev_ouv or output; n == 0; n_tris == 0; prev_poses with idx NULL, n_mesh == 0 or
 *      n_mesh > RTW_MAX_MESH_INSTANCES.
 *   3. rtw_temporal_accumulate_points is rtw_temporal_accumulate_motion plus prev_point and carried_normal, both [h][w][3] f32, both may be
 *      NULL.  A pixel HAS A POINT when prev_point != NULL and prev_point[p].x == prev_point[p].x.  For such a pixel
 *          P' = prev_point[p];  d = P' - prev_cam.origin;  s, fx, fy from d and the four taps as in "with a row" above (never the static
 *          shortcut's one tap); the normal test reads carried_normal[p] in place of normal[p] (carried_normal == NULL: normal[p] itself);
 *          its row, if any, is ignored.  An infinity or a NaN in P'.y or P'.z ends as an s or fx that is not finite: "no history".
 *      A pixel without a point follows "temporal accumulation with moving objects" byte for byte.  out_prev_xy as there.  The buffers may
 *      come from anywhere: a caller who skins or simulates geometry itself fills them without rtw_deform_motion.
 *      RTW_E_INVALID besides the refusals there: prev_point or carried_normal equal to out_color, out_moments, out_len, out_variance or
 *      out_prev_xy; carried_normal without prev_point.  With both NULL the calls are the _motion calls, launch for launch.
 * What stays out: a mesh whose topology changes (tri names another triangle), the moving spheres of ray.time, one fused launch for the
 * three passes.  There is no rtw_mgpu_* form and no JSON form. */
/* Host only, pure (one thread). */
int rtw_deform_motion(const int32_t *tri /* [n] */, const float *bary /* [n][2] */, uint32_t n, const float *prev_ouv /* [n_tris][9] */,
                      uint32_t n_tris, const int32_t *idx /* [n], with prev_poses */, const float *prev_poses /* [n_mesh][7] or NULL */,
                      uint32_t n_mesh, uint32_t first, float *prev_point_out /* [n][3] */, float *carried_normal_out /* [n][3] */);
/* On ctx's GPU, on its stream, blocking; the bytes of the host form, one thread per pixel.  Each buffer may independently be host memory
 * (staged; a result copied back) or device memory of ctx's GPU (used in place); the staging is kept, so a repeated size allocates nothing.
 * Needs no scene. */
int rtw_ctx_deform_motion(rtw_ctx *ctx, const int32_t *tri, const float *bary, uint32_t n, const float *prev_ouv, uint32_t n_tris,
                          const int32_t *idx, const float *prev_poses, uint32_t n_mesh, uint32_t first, float *prev_point_out,
                          float *carried_normal_out);
/* The host form (one thread) and, on ctx's GPU and stream, its bytes: a third instantiation of the kernel, chosen on the host. */
int rtw_temporal_accumulate_points(const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth, const float *normal,
                                   const int32_t *idx, const RtwCamera *prev_cam, const float *prev_color, const float *prev_moments,
                                   const float *prev_len, const float *prev_depth, const float *prev_normal, const int32_t *prev_idx,
                                   const RtwTemporal *params, const RtwMotionRow *rows /* may be NULL */, uint32_t n_rows, uint32_t first,
                                   const float *prev_point /* may be NULL */, const float *carried_normal /* may be NULL */,
                                   float *out_color, float *out_moments, float *out_len, float *out_variance /* may be NULL */,
                                   float *out_prev_xy /* may be NULL */, RtwFilterStats *stats);
int rtw_ctx_temporal_accumulate_points(rtw_ctx *ctx, const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth,
                                       const float *normal, const int32_t *idx, const RtwCamera *prev_cam, const float *prev_color,
                                       const float *prev_moments, const float *prev_len, const float *prev_depth,
                                       const float *prev_normal, const int32_t *prev_idx, const RtwTemporal *params,
                                       const RtwMotionRow *rows /* may be NULL */, uint32_t n_rows, uint32_t first,
                                       const float *prev_point /* may be NULL */, const float *carried_normal /* may be NULL */,
                                       float *out_color, float *out_moments, float *out_len, float *out_variance /* may be NULL */,
                                       float *out_prev_xy /* may be NULL */, RtwFilterStats *stats);

/* ---- variance estimate: a luminance variance for every pixel of an accumulated frame -- added within v4 ---------------------------------
 * SVGF's variance estimation (Schied et al. 2017, section 4.2): where the history is long enough the variance over time that the two
 * accumulated moments hold, elsewhere (a first frame, a disocclusion) a variance over space from the moments of the neighbours on the same
 * surface, raised by how short the history is.  moments [h][w][2] f32 and len [h][w] f32 are rtw_temporal_accumulate's out_moments and
 * out_len; depth, normal, idx the guides of the same frame, as the a-trous filter reads them; out [h][w] f32.  Everything is f32 with one
 * rounding per written operation (no fused multiply-add), exp_plain is rtw_exp_plain's.  Pixel p, n = len[p], (m1, m2) = moments[p]:
 *   n >= min_history:   V = m2 - m1*m1;  out[p] = V > 0 ? V : 0      (rtw_temporal_accumulate's out_variance, byte for byte)
 *   otherwise (also a NaN n):  the taps q = p + (dx, dy), dy = -radius..radius outer, dx = -radius..radius inner (the centre among them),
 *   skipping those outside the frame and those with !(len[q] > 0);  a = 0
 *     if sigma_depth  > 0:  dz = depth[q] - depth[p];    a = a + inv_depth * (dz * dz)
 *     if sigma_normal > 0:  d = normal[q] - normal[p];   a = a + inv_normal * ((d.x*d.x + d.y*d.y) + d.z*d.z)
 *     g = (a >= 0) ? exp_plain(-a) : 0;   if same_object and idx[q] != idx[p]:  g = 0
 *     if g > 0:  s1 = s1 + g * m1[q];  s2 = s2 + g * m2[q];  ws = ws + g
 *   (the a-trous filter's weight with its colour term off and its depth scale 1, inv_x = 0.5f / (sigma_x * sigma_x))
 *   ws > 0:   M1 = s1 / ws;  M2 = s2 / ws;  V = M2 - M1*M1;  V = V > 0 ? V : 0;  out[p] = V * ((float)min_history / (n >= 1 ? n : 1))
 *   else:     out[p] = 0
 * min_history == 1 sends every pixel with len >= 1 down the first branch: the spatial estimate is off.  A guide whose term is off may be
 * NULL and is never read.
 * RTW_E_INVALID, nothing written: moments, len, out or params NULL; w or h zero or beyond RTW_ATROUS_MAX_SIDE, or w * h beyond 32 bits;
 * min_history outside 1 .. 65535; radius outside 1 .. RTW_VARIANCE_MAX_RADIUS; a sigma that is negative or not finite, or so small that
 * its inv_* is not finite; sigma_depth > 0 with depth NULL, sigma_normal > 0 with normal NULL, same_object with idx NULL; same_object > 1;
 * out == moments or out == len (neighbours gather from both).  There is no rtw_mgpu_* form and no JSON form. */
#define RTW_VARIANCE_MAX_RADIUS 3u
typedef struct RtwVarianceEstimate {
    uint32_t min_history;           /* 1 .. 65535: a pixel with len below it takes the spatial estimate; 1 = never      */
    uint32_t radius;                /* 1 .. RTW_VARIANCE_MAX_RADIUS: the spatial window is (2 radius + 1)^2 pixels      */
    float    sigma_depth;           /* 0 = no depth term; else in the units of `depth`                                 */
    float    sigma_normal;          /* 0 = no normal term; else in units of |n - n'|                                   */
    uint32_t same_object;           /* 1 = a tap on another idx weighs 0                                               */
} RtwVarianceEstimate;
/* The host form (one thread).  RtwFilterStats: filter_ms and total_ms are the call's time, taps counts the window entries inside the
 * frame, the other fields are 0. */
int rtw_variance_estimate(const float *moments, const float *len, uint32_t w, uint32_t h, const float *depth, const float *normal,
                          const int32_t *idx, const RtwVarianceEstimate *params, float *out, RtwFilterStats *stats);
/* On ctx's GPU, on its stream, blocking; the bytes of the host form.  Every buffer may independently be host memory or device memory of
 * ctx's GPU (host memory is staged).  One launch, one thread per pixel, the window read from an LDS tile or from global memory
 * (RTW_OPT_ATROUS_LAYOUT); filter_ms is its device time.  Needs no scene and leaves the scene, and every render, untouched. */
int rtw_ctx_variance_estimate(rtw_ctx *ctx, const float *moments, const float *len, uint32_t w, uint32_t h, const float *depth,
                              const float *normal, const int32_t *idx, const RtwVarianceEstimate *params, float *out,
                              RtwFilterStats *stats);

/* ---- variance-steered a-trous filter: SVGF's filter stage -- added within v4 -----------------------------------------------------------
 * rtw_atrous_filter with a variance channel beside the colour (Schied et al. 2017, section 4.4): a luminance term whose width follows
 * the pixel's own variance, so that a pixel that has converged is left alone and a noisy one is filtered hard, and the variance itself
 * filtered by the squared weights so that the next level sees what the last one left.  variance [h][w] f32 is what rtw_variance_estimate
 * writes (the variance of the luminance of `in`); out_variance [h][w] f32 may be NULL.  Everything else is rtw_atrous_filter's, params
 * included: its sigma_color term stays available, and sigma_color = 0 steers by the variance alone.
 * With lum(c) = (0.2126f c.r + 0.7152f c.g) + 0.0722f c.b:
 *   demodulate:  C0 as rtw_atrous_filter;  la = lum(a) of its a_c (exactly 1 without albedo);
 *                V0[p] = variance[p] > 0 ? variance[p] / (la*la) : 0          (NaN and negatives become 0, +inf stays)
 *   level i, centre p, when sigma_luminance > 0:
 *     prefilter:  vbar = (sum G[|dx|] G[|dy|] Vi[q]) / (sum G[|dx|] G[|dy|]) over the q = p + (dx, dy) inside the frame, dy = -1..1
 *                 outer, dx = -1..1 inner, G = {1/2, 1/4}; the step is 1 at every level.  Without prefilter:  vbar = Vi[p]
 *     den = sl2 * vbar + epsilon,   sl2 = 2 * sigma_luminance * sigma_luminance formed once per call
 *   each of the 25 taps q:  a as rtw_atrous_filter forms it (colour, depth, normal, in this order), then
 *     if sigma_luminance > 0:  dl = lum(Ci[q]) - lum(Ci[p]);  a = a + (dl*dl) / den
 *     g, wt as rtw_atrous_filter;   if wt > 0:  its sums, and  vs = vs + (wt*wt) * Vi[q]
 *   Ci+1[p] as rtw_atrous_filter;   Vi+1[p] = wsum > 0 ? vs / (wsum*wsum) : Vi[p]
 *   remodulate:  out as rtw_atrous_filter;   out_variance[p] = V_levels[p] * (la*la)
 * The luminance term is Gaussian in dl, dl^2 / (2 sigma^2 v), where SVGF has |dl| / (sigma sqrt(v)): deliberately, so that it has the
 * shape of the other three terms and needs no square root.  With sigma_luminance = 0 `out` holds rtw_atrous_filter's bytes.
 * `out` may be `in`.
 * RTW_E_INVALID, nothing written: everything rtw_atrous_filter refuses; variance or vparams NULL; sigma_luminance negative or not finite,
 * or so large that sl2 is not finite; epsilon not finite or not > 0; prefilter > 1; out_variance == variance, in or out.
 * There is no rtw_mgpu_* form and no JSON form. */
typedef struct RtwSvgf {
    float    sigma_luminance;       /* 0 = no luminance term; else in standard deviations of the pixel's luminance      */
    float    epsilon;               /* > 0: added to the scaled variance, so that a variance of 0 does not divide by 0   */
    uint32_t prefilter;             /* 1 = the centre's variance is the 3 x 3 Gaussian mean of its neighbourhood         */
} RtwSvgf;
/* The host form (one thread).  RtwFilterStats as rtw_atrous_filter. */
int rtw_svgf_filter(const float *in, const float *variance, uint32_t w, uint32_t h, const float *depth, const float *normal,
                    const int32_t *idx, const float *albedo, const float *emitted, const RtwAtrous *params, const RtwSvgf *vparams,
                    float *out, float *out_variance /* may be NULL */, RtwFilterStats *stats);
/* On ctx's GPU, on its stream, blocking; the bytes of the host form; buffers as rtw_ctx_atrous_filter, whose scratch it shares and grows
 * by two variance planes.  One launch per level (RTW_OPT_ATROUS_LAYOUT); filter_ms is the device time of all launches. */
int rtw_ctx_svgf_filter(rtw_ctx *ctx, const float *in, const float *variance, uint32_t w, uint32_t h, const float *depth,
                        const float *normal, const int32_t *idx, const float *albedo, const float *emitted, const RtwAtrous *params,
                        const RtwSvgf *vparams, float *out, float *out_variance /* may be NULL */, RtwFilterStats *stats);

/* ---- neighbourhood colour bounds: mean +- k sigma of the frame around each pixel -- added within v4 --------------------------------------
 * The box that variance clipping clips a reprojected colour to ("bounded temporal accumulation" below), and, taken without the centre
 * pixel, the usual firefly clamp of the frame itself.  in, out_lo, out_hi and out_clamped (may be NULL) are [h][w][3] f32; idx [h][w] i32 as
 * rtw_ctx_surface_map writes it (may be NULL without same_object).  Everything is f32 with one rounding per written operation (no fused
 * multiply-add), the divide and sqrtf correctly rounded.  Pixel p:
 *   the taps q = p + (dx, dy), dy = -radius..radius outer, dx = -radius..radius inner, skipping those outside the frame; q == p with
 *   exclude_centre; those with idx[q] != idx[p] with same_object; those with a channel of in[q] that is not finite
 *   n = the taps that count, nf = (float)n
 *   n == 0:  lo_c = -inf, hi_c = +inf for the three channels
 *   else, per channel c, two sweeps over the counted taps in that order:
 *     s = s + in[q]_c;              mu = s / nf
 *     d = in[q]_c - mu;  qq = qq + d*d
 *     sd = sqrtf(qq / nf);  e = k * sd;  lo_c = mu - e;  hi_c = mu + e
 *   (two sweeps on purpose: beside values of 0.1 a firefly of 1e4 cancels away in s2/n - mu*mu)
 *   out_clamped[p]_c, x = in[p]_c:  x finite:  x < lo_c ? lo_c : (x > hi_c ? hi_c : x);   else x as it is
 * A NaN bound (a sum that overflowed, k = 0 beside an infinite sd) therefore clamps nothing and is no error.
 * RTW_E_INVALID, nothing written: in, params, out_lo or out_hi NULL; w or h zero or beyond RTW_ATROUS_MAX_SIDE, or w * h beyond 32 bits;
 * radius outside 1 .. RTW_BOUNDS_MAX_RADIUS; k negative or not finite; same_object > 1 or exclude_centre > 1; same_object with idx NULL;
 * two of the three outputs the same buffer; an output that is `in` (neighbours gather from it).
 * What stays out: boxes in YCoCg or of the luminance alone, bounds of a prefiltered frame, one launch fused with the accumulation.  There is
 * no rtw_mgpu_* form and no JSON form. */
#define RTW_BOUNDS_MAX_RADIUS 3u
typedef struct RtwColourBounds {
    uint32_t radius;          /* 1 .. RTW_BOUNDS_MAX_RADIUS: the window is (2 radius + 1)^2 pixels          */
    float    k;               /* >= 0, finite: the half-width of the box in standard deviations            */
    uint32_t same_object;     /* 1 = a tap on another idx is skipped                                       */
    uint32_t exclude_centre;  /* 1 = the pixel itself is not a tap (the firefly form)                      */
} RtwColourBounds;
/* The host form (one thread).  RtwFilterStats as rtw_variance_estimate: taps counts the window entries inside the frame. */
int rtw_colour_bounds(const float *in, uint32_t w, uint32_t h, const int32_t *idx /* may be NULL */, const RtwColourBounds *params,
                      float *out_lo, float *out_hi, float *out_clamped /* may be NULL */, RtwFilterStats *stats);
/* On ctx's GPU, on its stream, blocking; the bytes of the host form.  Every buffer may independently be host memory (staged through a
 * scratch the context keeps) or device memory of ctx's GPU (used in place).  One launch, one thread per pixel, the window read from an
 * LDS tile or from global memory (RTW_OPT_ATROUS_LAYOUT); filter_ms is its device time.  Needs no scene. */
int rtw_ctx_colour_bounds(rtw_ctx *ctx, const float *in, uint32_t w, uint32_t h, const int32_t *idx /* may be NULL */,
                          const RtwColourBounds *params, float *out_lo, float *out_hi, float *out_clamped /* may be NULL */,
                          RtwFilterStats *stats);

/* ---- bounded temporal accumulation: the history's colour clipped to a box before it is blended -- added within v4 -------------------------
 * The geometric tests accept a history however stale its lighting is.  rtw_temporal_accumulate_bounded is rtw_temporal_accumulate_points
 * plus hist_lo and hist_hi, both [h][w][3] f32, both or neither NULL, and out_clipped [h][w] f32 (may be NULL).  For a pixel p with a
 * history (the counted taps' weight > 0), directly after h = (the taps' colour) / (their weight) and before it is blended or kept:
 *     h'_c = h_c < lo_c ? lo_c : (h_c > hi_c ? hi_c : h_c),   lo = hist_lo[p], hi = hist_hi[p]      (a NaN bound clips nothing)
 *     out_clipped[p] = (|h_0 - h'_0| + |h_1 - h'_1|) + |h_2 - h'_2|
 * and h' takes the place of h.  The moments and the length are the unbounded call's: a pixel whose lighting changed keeps a large variance,
 * which the variance-steered filter then filters harder.  A pixel without a history reads no bound and writes out_clipped[p] = 0, as every
 * pixel of a first frame does.  The bounds may come from anywhere: rtw_colour_bounds of the new frame, a prefiltered frame, an analytic box.
 * RTW_E_INVALID besides the refusals of the _points call: exactly one of hist_lo and hist_hi; hist_lo, hist_hi or out_clipped equal to
 * out_color, out_moments, out_len, out_variance or out_prev_xy; out_clipped equal to hist_lo or hist_hi.  With all three NULL the calls
 * are the _points calls, launch for launch.
 * What stays out: a response of the history length or of the moments to clipping.  There is no rtw_mgpu_* form and no JSON form. */
/* The host form (one thread) and, on ctx's GPU and stream, its bytes: a fourth instantiation of the kernel, chosen on the host. */
int rtw_temporal_accumulate_bounded(const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth, const float *normal,
                                    const int32_t *idx, const RtwCamera *prev_cam, const float *prev_color, const float *prev_moments,
                                    const float *prev_len, const float *prev_depth, const float *prev_normal, const int32_t *prev_idx,
                                    const RtwTemporal *params, const RtwMotionRow *rows /* may be NULL */, uint32_t n_rows, uint32_t first,
                                    const float *prev_point /* may be NULL */, const float *carried_normal /* may be NULL */,
                                    const float *hist_lo /* may be NULL */, const float *hist_hi /* may be NULL */,
                                    float *out_color, float *out_moments, float *out_len, float *out_variance /* may be NULL */,
                                    float *out_prev_xy /* may be NULL */, float *out_clipped /* may be NULL */, RtwFilterStats *stats);
int rtw_ctx_temporal_accumulate_bounded(rtw_ctx *ctx, const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth,
                                        const float *normal, const int32_t *idx, const RtwCamera *prev_cam, const float *prev_color,
                                        const float *prev_moments, const float *prev_len, const float *prev_depth,
                                        const float *prev_normal, const int32_t *prev_idx, const RtwTemporal *params,
                                        const RtwMotionRow *rows /* may be NULL */, uint32_t n_rows, uint32_t first,
                                        const float *prev_point /* may be NULL */, const float *carried_normal /* may be NULL */,
                                        const float *hist_lo /* may be NULL */, const float *hist_hi /* may be NULL */,
                                        float *out_color, float *out_moments, float *out_len, float *out_variance /* may be NULL */,
                                        float *out_prev_xy /* may be NULL */, float *out_clipped /* may be NULL */, RtwFilterStats *stats);

/* ---- guided upsampling: a low-resolution frame reconstructed at the output size from full-size guides -- added within v4 -------------------
 * Joint bilateral upsampling (Kopf et al. 2007) on demodulated colour: the expensive samples are traced on a grid `scale` times coarser, the
 * guides (which cost almost nothing) at both sizes, and texture and silhouettes come from the output-size guides at full sharpness.
 * `lo` is a linear f32 frame [h_lo][w_lo][3]; one RtwGuides is at the low size and one at the output size [h][w], both in the layouts
 * rtw_ctx_surface_map writes: depth f32, normal [..][3] f32, idx i32, albedo [..][3] f32, emitted [..][3] f32.  scale = s is in
 * 1 .. RTW_UPSAMPLE_MAX_SCALE, w_lo == ceil(w / s), h_lo == ceil(h / s); low pixel (I, J) covers output pixels s*I .. s*I+s-1 by
 * s*J .. s*J+s-1 (rtw_camera_scaled gives the camera whose pixels those are).  Everything is f32 with one rounding per written operation
 * (no fused multiply-add), exp_plain is rtw_exp_plain's:
 *   demodulate, at a low pixel q:  a_c = (albedo_lo && albedo_lo[q][c] >= albedo_floor) ? albedo_lo[q][c] : 1;
 *                e_c = emitted_lo ? emitted_lo[q][c] : 0;   L[q][c] = (lo[q][c] - e_c) / a_c
 *   footprint of output pixel p = (i, j), formed in integers:  N = 2*i + 1 - s, D = 2*s;  I0 = floor(N / D) (floor division: -1 on the
 *                first columns);  tx = (float)(N - I0*D) / (float)D;  J0 and ty likewise from j
 *   taps ky = -(radius-1) .. radius outer, kx likewise inner, radius 1 or 2 (2 x 2 or 4 x 4 low pixels):  q = (I0 + kx, J0 + ky), those
 *   outside the low frame skipped;  wx = kx <= 0 ? (float)(radius + kx) - tx : (float)(radius - kx) + tx, wy likewise;  hw = wx * wy
 *   (a tent; the bilinear weights at radius 1);  a = 0
 *     if sigma_depth  > 0:  dz = (depth_lo[q] - depth_hi[p]) * inv_s;  a = a + inv_depth * (dz * dz)        inv_s = 1.0f / (float)s
 *     if sigma_normal > 0:  d = normal_lo[q] - normal_hi[p];           a = a + inv_normal * ((d.x*d.x + d.y*d.y) + d.z*d.z)
 *     g = (a >= 0) ? exp_plain(-a) : 0;   if same_object and idx_lo[q] != idx_hi[p]:  g = 0;   wt = hw * g
 *     if wt > 0 and L[q][0], L[q][1], L[q][2] are all finite:  sum_c = sum_c + L[q][c] * wt;  wsum = wsum + wt
 *   C = wsum > 0 ? sum / wsum : L[(i / s, j / s)]         (the fallback: the covering low pixel, unguided; a NaN there passes through)
 *   remodulate:  out[p][c] = C_c * ah_c + eh_c, ah_c and eh_c by the same floor rule from albedo_hi and emitted_hi
 * with inv_x = 0.5f / (sigma_x * sigma_x) as in the a-trous filter.  wsum_out [h][w] f32 (may be NULL) receives every pixel's wsum: 0 exactly
 * where the fallback was taken, the pass's diagnostic as out_clipped is the bounded accumulation's.  A guide whose term is off, and any
 * albedo or emitted buffer, may be NULL and is then never read; guides_lo or guides_hi NULL is a struct of NULLs.
 * RTW_E_INVALID, nothing written: lo, out or params NULL; w or h zero or beyond RTW_ATROUS_MAX_SIDE, or w * h beyond 32 bits; a low size that
 * is not the ceiling above; scale outside 1 .. RTW_UPSAMPLE_MAX_SCALE or radius outside 1 .. RTW_UPSAMPLE_MAX_RADIUS; a sigma that is
 * negative or not finite, or so small that its inv_* is not finite; a term that is on with its guide NULL on either side; same_object > 1;
 * with an albedo given on either side, an albedo_floor that is not finite or not > 0; out or wsum_out equal to a buffer that is read, or to
 * each other.  `out` must not overlap an input in any other way either.
 * What stays out: a plane-distance depth term, fractional scales, a colour term, upsampling of a history.  There is no rtw_mgpu_* form and
 * no JSON form. */
#define RTW_UPSAMPLE_MAX_SCALE  8u
#define RTW_UPSAMPLE_MAX_RADIUS 2u
typedef struct RtwGuides {
    const float   *depth;           /* [..] f32                                                                       */
    const float   *normal;          /* [..][3] f32                                                                    */
    const int32_t *idx;             /* [..] i32                                                                       */
    const float   *albedo;          /* [..][3] f32, may be NULL whatever the terms                                    */
    const float   *emitted;         /* [..][3] f32, may be NULL whatever the terms                                    */
} RtwGuides;
typedef struct RtwUpsample {
    uint32_t scale;                 /* 1 .. RTW_UPSAMPLE_MAX_SCALE: output pixels per low pixel along a side          */
    uint32_t radius;                /* 1 = 2 x 2 low pixels (bilinear), 2 = 4 x 4 (a tent)                            */
    float    sigma_depth;           /* 0 = no depth term; else in the units of `depth` per low pixel                  */
    float    sigma_normal;          /* 0 = no normal term; else in units of |n - n'|                                  */
    uint32_t same_object;           /* 1 = a tap on another idx weighs 0                                             */
    float    albedo_floor;          /* used when an albedo is given: a channel below it is not (de/re)modulated       */
} RtwUpsample;
/* The host form (one thread).  RtwFilterStats: filter_ms and total_ms are the call's time, taps counts the taps inside the low frame, the
 * other fields are 0. */
int rtw_upsample_filter(const float *lo, uint32_t w_lo, uint32_t h_lo, const RtwGuides *guides_lo, uint32_t w, uint32_t h,
                        const RtwGuides *guides_hi, const RtwUpsample *params, float *out, float *wsum_out /* may be NULL */,
                        RtwFilterStats *stats);
/* On ctx's GPU, on its stream, blocking; the bytes of the host form.  Every buffer may independently be host memory (staged through a
 * scratch the context keeps) or device memory of ctx's GPU (used in place).  One launch, one thread per output pixel, the low window read
 * from an LDS tile or from global memory (RTW_OPT_ATROUS_LAYOUT); filter_ms is its device time.  Needs no scene. */
int rtw_ctx_upsample_filter(rtw_ctx *ctx, const float *lo, uint32_t w_lo, uint32_t h_lo, const RtwGuides *guides_lo, uint32_t w, uint32_t h,
                            const RtwGuides *guides_hi, const RtwUpsample *params, float *out, float *wsum_out /* may be NULL */,
                            RtwFilterStats *stats);
/* Host only, pure: the camera whose pixel (I, J) is the scale x scale block of cam's pixels.  delta_u and delta_v are multiplied by
 * (float)scale, every other field is copied (nothing goes back through vfov): its ray at offset (0.5, 0.5) is cam's at
 * (scale*I + scale/2, scale*J + scale/2).  Render and take the low guides with it at ceil(w / scale) x ceil(h / scale), for any size.
 * RTW_E_INVALID for NULL or a scale outside 1 .. RTW_UPSAMPLE_MAX_SCALE. */
int rtw_camera_scaled(const RtwCamera *cam, uint32_t scale, RtwCamera *out);

/* ---- display stage: luminance histogram, exposure from it, tone map / transfer / bytes -- added within v4 ----------------------------------
 * The last steps from a linear f32 frame [h][w][3] to something to look at.  Three calls: a histogram of the frame's luminance (a kernel),
 * an exposure metered from that histogram (pure host code), and the display transform (a kernel).  Everything per pixel is f32 with one
 * rounding per written operation (no fused multiply-add), divides correctly rounded, pow_plain (rtw_pow_plain) the only elementary function.
 *
 * 1. rtw_luminance_histogram.  Per pixel  Y = (0.2126f * r + 0.7152f * g) + 0.0722f * b,  and exactly one of
 *      non-finite:  a channel is NaN or infinite, or Y overflowed to +inf          -> counts[1]
 *      black:       finite channels and Y <= 0 (a Y that overflowed to -inf too)   -> counts[0]
 *      counted:     bin = clamp((int)(bits(Y) >> 20) - 888, 0, 255)                -> hist[bin]
 *    bits(Y) >> 20 is the exponent and the top three mantissa bits: eight bins a stop over 2^-16 .. 2^16, linear in the mantissa within a stop;
 *    subnormals and everything below 2^-16 land in bin 0, everything from 2^16 up in bin 255.  hist is uint32[256], counts uint32[2];
 *    sum(hist) + counts[0] + counts[1] == w * h.  The counts are integers: the host form and the kernel agree exactly.
 *    RTW_E_INVALID, nothing written: in, hist or counts NULL; w or h zero or beyond RTW_ATROUS_MAX_SIDE, or w * h beyond 32 bits; hist or counts
 *    overlapping `in` or each other.
 *
 * 2. rtw_exposure_from_histogram.  Host only, pure, double arithmetic, no libm call.  With N = sum(hist):
 *      drop the floor(N * low_permille / 1000) lowest and the floor(N * high_permille / 1000) highest counted pixels, in integers (a bin can
 *      be cut in part);  over the n left:  S = sum c_i (2 i + 1) in uint64,  m = S / (2 n): the mean bin position, a bin's pixels at its centre;
 *      m = clamp(m, min_level, max_level);   level = prev_level + rate * (m - prev_level), or m when prev_level is NaN (a first frame);
 *      back through the inverse of the bin rule:  s = floor(level / 8),  f = level / 8 - s,  Ymeter = (1 + f) * 2^(s - 16),
 *      exposure = (float)(key / Ymeter).
 *    n == 0 (nothing counted):  level = prev_level and exposure = prev_exposure, or 1 when prev_level is NaN.
 *    The mean and its inverse both live in the bin rule's piecewise-linear logarithm (1 + f for 2^f), which no elementary function enters: a
 *    float64 restatement gives the same bits.  Against a true mean of log2 Y the metered level is off by at most 0.086 stops (the largest gap
 *    between log2(1 + f) and f), which for metering is irrelevant.
 *    RTW_E_INVALID, nothing written: a NULL; low_permille + high_permille >= 1000; key not finite or not > 0; rate outside [0, 1]; min_level or
 *    max_level outside [0, 256] or min_level > max_level; a prev_level that is neither NaN nor in [0, 256].
 *
 * 3. rtw_display.  Per pixel (i, j), per channel c:
 *      x = in_c * exposure
 *      tone NONE:           v = x
 *           REINHARD:       v = (x * (1.0f + x / (white * white))) / (1.0f + x)
 *           REINHARD_LUMA:  Y = (0.2126f * x_r + 0.7152f * x_g) + 0.0722f * x_b;   T = (Y * (1.0f + Y / (white * white))) / (1.0f + Y);
 *                           v_c = Y > 0 ? x_c * (T / Y) : x_c
 *           ACES_FIT:       v = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f)                       (Narkowicz 2016)
 *      clamp:               v = v != v ? v : (v < 0 ? 0 : (v > 1 ? 1 : v))                                          (a NaN propagates)
 *      transfer GAMMA:      v = pow_plain(v, inv_gamma),  inv_gamma = 1.0f / gamma formed on the host; no call when inv_gamma == 1.0f
 *               SRGB:       v = v <= 0.0031308f ? 12.92f * v : 1.055f * pow_plain(v, 0.4166666567325592f) - 0.055f   (the f32 of 1 / 2.4)
 *      out_format F32:      out_c = v
 *      bytes, dither 0:     t = v * scale;  t = t != t ? t : (t < 0 ? 0 : (t > 255 ? 255 : t));  byte = NaN ? 0 : round half away from zero
 *                           -- rtw_quantize_u8 with quantise RUST (scale 255.0f), rtw_quantize_u8_rust2 with RUST2 (scale 255.99f)
 *      bytes, dither 1:     t as above;  d = ((float)B[j & 7][i & 7] + 0.5f) * 0.015625f;  byte = NaN ? 0 : min(255, (int)floorf(t + d))
 *    with B the 8 x 8 Bayer matrix
 *        0 32  8 40  2 34 10 42 / 48 16 56 24 50 18 58 26 / 12 44  4 36 14 46  6 38 / 60 28 52 20 62 30 54 22 /
 *        3 35 11 43  1 33  9 41 / 51 19 59 27 49 17 57 25 / 15 47  7 39 13 45  5 37 / 63 31 55 23 61 29 53 21      (rows j & 7 = 0 .. 7)
 *    out is [h][w][3] uint8 (RGB8), [h][w][4] uint8 with alpha 255 (RGBA8) or [h][w][3] f32 (F32).
 *    RTW_E_INVALID, nothing written: in, params or out NULL; sizes as above; exposure not finite or negative; gamma not finite or not > 0, or
 *    so small that 1.0f / gamma is not finite; white not finite or not > 0 under a Reinhard form; tone, transfer, quantise or out_format out
 *    of range; dither > 1; out overlapping in (F32 in place too: one rule).
 * What stays out: local tone mapping, a BGRA or 10-bit output, an exposure that stays on the device (the calls block, and the histogram
 * is 1 KB).  There is no rtw_mgpu_* form and no JSON form. */
enum { RTW_TONE_NONE = 0, RTW_TONE_REINHARD = 1, RTW_TONE_REINHARD_LUMA = 2, RTW_TONE_ACES_FIT = 3 };
enum { RTW_TRANSFER_GAMMA = 0, RTW_TRANSFER_SRGB = 1 };
enum { RTW_QUANTISE_RUST = 0, RTW_QUANTISE_RUST2 = 1 };
enum { RTW_DISPLAY_RGB8 = 0, RTW_DISPLAY_RGBA8 = 1, RTW_DISPLAY_F32 = 2 };
typedef struct RtwMetering {
    uint32_t low_permille;    /* the share of the darkest counted pixels left out, in 1/1000                */
    uint32_t high_permille;   /* ... and of the brightest; low + high < 1000                                */
    float    key;             /* > 0: the luminance the metered level maps to (0.18: middle grey)           */
    float    rate;            /* 0 .. 1: the step towards this frame's level; 1 = no adaptation             */
    float    min_level;       /* the metered level is clamped to [min_level, max_level], in bins (0 .. 256) */
    float    max_level;
} RtwMetering;
typedef struct RtwDisplay {
    float    exposure;        /* >= 0, finite                                                               */
    uint32_t tone;            /* RTW_TONE_*                                                                 */
    float    white;           /* the Reinhard forms: the luminance that maps to 1                           */
    uint32_t transfer;        /* RTW_TRANSFER_*                                                             */
    float    gamma;           /* > 0, finite; read under RTW_TRANSFER_GAMMA, checked always                 */
    uint32_t quantise;        /* RTW_QUANTISE_*                                                             */
    uint32_t dither;          /* 0 or 1                                                                     */
    uint32_t out_format;      /* RTW_DISPLAY_*                                                              */
} RtwDisplay;
/* The host forms (one thread).  RtwFilterStats: filter_ms and total_ms are the call's time, taps is w * h, the other fields are 0. */
int rtw_luminance_histogram(const float *in, uint32_t w, uint32_t h, uint32_t *hist /* [256] */, uint32_t *counts /* [2] */,
                            RtwFilterStats *stats);
int rtw_exposure_from_histogram(const uint32_t *hist /* [256] */, const RtwMetering *metering, double prev_level /* NaN: a first frame */,
                                float prev_exposure, double *level_out, float *exposure_out);
int rtw_display(const float *in, uint32_t w, uint32_t h, const RtwDisplay *params, void *out, RtwFilterStats *stats);
/* On ctx's GPU, on its stream, blocking; the bytes of the host forms.  Every buffer may independently be host memory (staged through a
 * scratch the context keeps) or device memory of ctx's GPU (used in place); filter_ms is the kernel's device time.  They need no scene.
 * The histogram is a grid-stride loop of at most RTW_HISTOGRAM_BLOCKS_PER_CU workgroups a compute unit, each pass of a workgroup taking
 * RTW_HISTOGRAM_BLOCK_PIXELS pixels, counted in LDS and added to a zeroed device buffer once per non-empty slot and workgroup
 * (RTW_OPT_HISTOGRAM_COUNT chooses how the LDS counts are kept).  The display transform is one thread per four consecutive pixels.  Both read
 * 16 bytes at a time when `in` is 16-byte aligned (and `out` 4-byte aligned for RGB8, 16-byte aligned for RGBA8 and F32) and pixel by pixel
 * otherwise and for the last w * h % 4 pixels. */
#define RTW_HISTOGRAM_BLOCKS_PER_CU 4u
#define RTW_HISTOGRAM_BLOCK_PIXELS  1024u
int rtw_ctx_luminance_histogram(rtw_ctx *ctx, const float *in, uint32_t w, uint32_t h, uint32_t *hist /* [256] */, uint32_t *counts /* [2] */,
                                RtwFilterStats *stats);
int rtw_ctx_display(rtw_ctx *ctx, const float *in, uint32_t w, uint32_t h, const RtwDisplay *params, void *out, RtwFilterStats *stats);

/* ---- bloom: bright pass, dual-filter pyramid, composite -- added within v4 ------------------------------------------------------------------
 * The glare of what is far above 1, on the linear f32 frame [h][w][3] in front of the display stage: a neighbourhood operation, where the
 * display transform is a function of one pixel.  Everything is f32 with one rounding per written operation (no fused multiply-add), divides
 * correctly rounded, no elementary function; sums run in the written order.
 *
 * Sizes.  Level 0 is the frame.  Level l + 1 has w' = (w_l + 1) / 2, h' = (h_l + 1) / 2; its pixel (I, J) sits over pixels 2I, 2I + 1 by
 * 2J, 2J + 1 of level l.  A call asks for `levels` in 1 .. RTW_BLOOM_MAX_LEVELS; the chain stops early at the first level that is 1 x 1.
 * rtw_bloom_levels (host only, pure) returns the number n of levels used and, when sizes is not NULL, w and h of levels 1 .. n; 0 for a w or
 * h of zero or levels outside 1 .. RTW_BLOOM_MAX_LEVELS.
 *
 * Bright pass, per pixel x = (r, g, b) of level 0:
 *      usable:  all three channels finite       (a pixel that is not usable is a tap of weight 0: a NaN or an infinity never spreads)
 *      x_c = x_c < 0 ? 0 : x_c
 *      Y = (0.2126f * x_r + 0.7152f * x_g) + 0.0722f * x_b                                      (the display stage's luminance)
 *      s = Y - threshold
 *      c = (knee > 0 && s > -knee && s < knee) ? ((s + knee) * (s + knee)) / (4.0f * knee) : (s > 0 ? s : 0)
 *      b_c = Y > 0 ? x_c * (c / Y) : 0
 *      kw  = karis ? 1.0f / (1.0f + ((0.2126f * b_r + 0.7152f * b_g) + 0.0722f * b_b)) : 1.0f
 *    The quadratic meets max(s, 0) at both ends of the knee; with knee <= threshold c <= Y up to rounding, so b is finite whenever x is and Y
 *    did not overflow.  kw is the Karis weight: it keeps one firefly from becoming a disc.
 *
 * Down, level l to l + 1, pixel (I, J): the taps are the pixels (2I + a, 2J + b) of level l, a, b = -2 .. 3, b the outer loop; a tap
 * outside level l is skipped.  D[b + 2][a + 2] is
 *        1 1 2 2 1 1 / 1 5 6 6 5 1 / 2 6 8 8 6 2 / 2 6 8 8 6 2 / 1 5 6 6 5 1 / 1 1 2 2 1 1                       (sum 128)
 * -- the 13-tap downsample of Jimenez (SIGGRAPH 2014), a centre box at 1/2 and four corner boxes at 1/8 of bilinear fetches at pixel corners,
 * as the 36 pixel weights it amounts to.
 *      wt = (D / 128.0f) * kw            (kw of the tap in the first step, where a tap that is not usable adds nothing; 1.0f afterwards)
 *      sum_c = sum_c + v_c * wt;  wsum = wsum + wt            (v = b of the bright pass in the first step, the level's pixel afterwards)
 *      level[l + 1][(I, J)] = wsum > 0 ? sum / wsum : 0
 *    The first step applies the bright pass to each tap as it reads it: no thresholded frame is ever stored.
 *
 * Up, in place over the down chain, from the last level to level 1:   level[l][p] = level[l][p] + spread * U(level[l + 1], p).
 * U at pixel (i, j) of the finer level:  N = 2i - 1,  I0 = floor(N / 4) (-1 at i = 0),  r = N - 4 I0 (1 or 3);  the columns are I0 - 1 + k,
 * k = 0 .. 3, weighted wx = {3, 7, 5, 1} when r == 1 and {1, 5, 7, 3} when r == 3;  the rows likewise from j;
 *      wt = (float)(wx[kx] * wy[ky]) / 256.0f,  rows outer, columns inner;  a tap outside the coarser level is skipped;  U = sum / wsum
 *    -- a 3 x 3 tent on the coarse level, then the bilinear fetch at the fine pixel's centre, multiplied out.  wsum > 0 always.
 *
 * Composite:  B = U(level[1], p) at level 0;  out[p][c] = in[p][c] + intensity * B_c;  layer_out[p][c] = B_c when layer_out is given.  A pixel
 * of `in` that is not finite passes through by the arithmetic.  out may be in.
 *
 * RTW_E_INVALID, nothing written: in, out or params NULL; w or h zero or beyond RTW_ATROUS_MAX_SIDE, or w * h beyond 32 bits; levels outside
 * 1 .. RTW_BLOOM_MAX_LEVELS; threshold, knee, spread or intensity negative or not finite; knee > threshold; karis > 1; layer_out overlapping
 * in or out; out overlapping in other than being equal to it.
 * The rule is total: finite channels so large that a sum or Y rounds to an infinity give what the arithmetic above gives.
 * What stays out: one workgroup for the tail of small levels, lens dirt and anamorphic streaks, a threshold that follows the exposure on the
 * device, threads in the host form.  There is no rtw_mgpu_* form and no JSON form. */
#define RTW_BLOOM_MAX_LEVELS 8u
typedef struct RtwBloom {
    uint32_t levels;          /* 1 .. RTW_BLOOM_MAX_LEVELS                                                  */
    float    threshold;       /* >= 0, finite: the luminance where the bright pass opens                    */
    float    knee;            /* 0 .. threshold: the half-width of the quadratic around it                  */
    uint32_t karis;           /* 0 or 1: the first down step weights a tap by 1 / (1 + its luminance)       */
    float    spread;          /* >= 0, finite: what a level takes of the coarser one on the way up          */
    float    intensity;       /* >= 0, finite: what the frame takes of the layer                            */
} RtwBloom;
uint32_t rtw_bloom_levels(uint32_t w, uint32_t h, uint32_t levels, uint32_t *sizes /* [2 * RTW_BLOOM_MAX_LEVELS]: w, h of levels 1 .. n; may be NULL */);
/* The host form (one thread, a pyramid of its own).  RtwFilterStats: filter_ms and total_ms are the call's time, taps counts the taps inside
 * their level over all steps, the other fields are 0. */
int rtw_bloom(const float *in, uint32_t w, uint32_t h, const RtwBloom *params, float *out, float *layer_out /* may be NULL */,
              RtwFilterStats *stats);
/* On ctx's GPU, on its stream, blocking; the bytes of the host form.  Every buffer may independently be host memory (staged) or device memory
 * of ctx's GPU (used in place); the pyramid is a scratch the context keeps.  2 n launches for n levels used, one thread per output pixel in
 * workgroups of 16 x 16, each reading its source window from an LDS tile or from global memory (RTW_OPT_ATROUS_LAYOUT); filter_ms is the
 * device time from before the first launch to after the last.  Needs no scene. */
int rtw_ctx_bloom(rtw_ctx *ctx, const float *in, uint32_t w, uint32_t h, const RtwBloom *params, float *out, float *layer_out /* may be NULL */,
                  RtwFilterStats *stats);

/* ---- Rust2 triangles (Rust2/src/objects/triangle.rs) ----------------------------------------------------------------------------
 * `Triangle{origin, u, v, mat, texture}` with the derived fields of Triangle::new (:28-50): n = u x v, normal = unit(n),
 * d = normal . origin, w = n / (n . n); the hit test of get_hit (:95-124) restated operation by operation in f32: reject when
 * |normal . dir| <= 1e-8 or t < mint || t > maxt (t = (d - normal . o) / (normal . dir)); point = o + dir t, planar = point - origin,
 * alfa = w . (planar x v), beta = w . (u x planar), reject when alfa < 0 || beta < 0 || alfa + beta > 1.  The normal is never flipped.
 * NaN falls through as in the reference: a degenerate triangle (u x v == 0) has a NaN normal and reports a NaN-t hit for every ray.
 * Extension of this library (Rust/ has no triangles): Scene::collision_normal stays spheres, quads, instances; the triangles come LAST, as
 * one more group: the closest triangle in list order (a later one replaces the current one only when strictly closer, the quad rule), and
 * that one replaces the result so far only when strictly closer.  Material inline as in RtwQuad; no velocity (Rust2's triangle has none).
 * tex < 0: the constant colour tex_color and `emitted` (ConstColorTexture, Rust2/src/objects/texture.rs:13-31); tex >= 0 under
 * RTW_INTEGRATOR_RUST2: Rust2's ImageTexture::color_at(alfa, beta) (Rust2/src/objects/texture.rs:94-105, emission image from
 * RtwTexture.emit_tex, else `emitted`); under every other integrator the quad's texel rule at (alfa, beta) (Rust/src/objects/quad.rs:64-79,
 * the texel times 1.0) and `emitted`.  alfa, beta are those of the hit point r.at(t) (Triangle::color, :130-136).  The derived fields are written by rtw_triangle_new and recomputed by the library from origin /
 * u / v wherever it reads triangles (rtw_ctx_set_triangles, rtw_triangle_hits). */
typedef struct RtwTriangle {
    float origin[3];
    float u[3];
    float v[3];
    float normal[3];      /* derived: unit(u x v)        */
    float d;              /* derived: normal . origin    */
    float w[3];           /* derived: n / (n . n)        */
    float tex_color[3];
    float metallicness;
    float opacity;
    float ir;
    float emitted[3];
    int32_t tex;          /* index into RtwScene.textures, or -1 */
} RtwTriangle;
/* Triangle::new with ConstColorTexture(color) (tex = -1) or textures[tex]: mat3 == NULL -> the quad default, emitted == NULL -> 0. */
int rtw_triangle_new(const float origin[3], const float u[3], const float v[3], const float *mat3, const float *emitted,
                     const float color[3], int32_t tex, RtwTriangle *out);
/* The triangles of the scene of the last rtw_ctx_set_scene (which clears them): uploads them and builds their BVH (a binned-SAH tree, leaves
 * of <= 4 triangles, global memory).  tris == NULL with n == 0 clears them.  RTW_E_NO_SCENE before any scene; RTW_E_INVALID for a tex
 * beyond the scene's textures; RTW_E_UNSUPPORTED while texture noise is set (and rtw_ctx_set_texture_noise with triangles set fails alike).
 * RTW_ACCEL_BRUTE renders walk the triangle list, RTW_ACCEL_BVH renders use the tree -- the same image bit for bit (DESIGN.md "Rust2
 * triangles"): the tree only prunes, with boxes inflated by the rounding bound, ties to the lower index.  Where that bound cannot hold the
 * list is walked instead: a triangle with a non-finite derived field, a coordinate beyond 2^40, |w| beyond 2^40 or an ill-conditioned shape
 * (max(|u|,|v|)^2 / |u x v| > 256); non-finite mint / maxt or beyond 2^40; per ray, an origin or direction that is not finite or with
 * |o| + |d| max(|mint|, |maxt|) beyond 2^40.  RtwStats.quad_tests counts the triangle tests too, RtwStats.node_tests the triangle-tree node
 * visits.  The one-shot rtw_render / rtw_render_multi_gpu carry no triangles. */
int rtw_ctx_set_triangles(rtw_ctx *ctx, const RtwTriangle *tris, uint32_t n);
int rtw_mgpu_set_triangles(rtw_mgpu *m, const RtwTriangle *tris, uint32_t n);
/* Host self-check of the tree rtw_ctx_set_triangles builds (no GPU): every triangle reachable exactly once, each leaf box contains its
 * triangles' inflated boxes, each node box its children's, skip links well formed.  RTW_OK or RTW_E_INVALID.  Optional outputs: node count,
 * depth, and list_walk = 1 when the triangles fall back to the list walk (a condition above). */
int rtw_triangle_bvh_validate(const RtwTriangle *tris, uint32_t n, uint32_t *n_nodes, uint32_t *depth, uint32_t *list_walk);
/* Closest-hit queries against the triangles alone, for tests and tools.  rays: [n_rays][6] = origin, direction.  t_out[i] = the t of the
 * closest triangle (the group rule above), idx_out[i] = its index in the list, or -1 (t_out = +inf) when none.  The host form walks the list;
 * the device form runs the device functions the render kernels call on the context's triangles, the list walk (RTW_ACCEL_BRUTE) or the
 * tree (RTW_ACCEL_BVH); host buffers in and out, blocking.  RTW_E_NO_SCENE when the context has no triangles. */
int rtw_triangle_hits(const RtwTriangle *tris, uint32_t n, const float *rays, uint32_t n_rays, float mint, float maxt,
                      float *t_out, int32_t *idx_out);
int rtw_ctx_triangle_hits(rtw_ctx *ctx, const float *rays, uint32_t n_rays, float mint, float maxt, uint32_t accel,
                          float *t_out, int32_t *idx_out, RtwStats *stats);

/* ---- scene ray queries and Rust2's depth_map (Rust2/src/viewport.rs:62-85) -------------------------------------------------------
 * One closest-hit query per ray against the WHOLE scene of a context -- the spheres, quads and instances of rtw_ctx_set_scene and the
 * triangles of rtw_ctx_set_triangles -- with no path around it: t, the top-level object and the normal of the first surface, for depth,
 * object-id and normal buffers (a guide for the bilateral filter, picking, debugging a scene).
 * The top-level object index counts spheres first, then quads, then instances, then triangles: a triangle k is reported as
 * n_spheres + n_quads + n_instances + k.  The tie rule is Scene::collision_normal's, the render's: within a group the first of equal t in
 * list order wins, a later group replaces an earlier one only when strictly closer.  RTW_ACCEL_BVH (the sphere tree and the triangle
 * tree, under the conditions a render puts on them, RTW_OPT_LIST_WALK_MAX included) returns the same t, index and normal as
 * RTW_ACCEL_BRUTE bit for bit, ties included.  The direction is used as given, NOT normalised: t is in units of |d|.  `time` is the
 * ray.time: a moving sphere is at centre + velocity * time.  The normal is the outward geometric normal of the render's hit record (sphere:
 * unit(point - centre); quad and triangle: the stored normal, never flipped; instance member: the member's, rotated into the world).
 * CONSTANT-DENSITY INSTANCES ARE SKIPPED: their hit is a random scattering distance and a query has no sample stream, so the answer is
 * the first SOLID surface; such an instance keeps its index slot (the other indices do not shift) and is never reported.
 * No host implementation (the library has no CPU path for sphere, quad or instance hits) and no rtw_mgpu_* form. */
/* Host only, pure: the rays of Viewport::depth_map for Rust2's camera (rtw_camera2_new: pixel00 = left_top, delta_u / delta_v = the
 * full-viewport delta_x / delta_y).  Pixel (i, j), row-major at rays_out[(j * width + i) * 6]: origin = cam.origin, direction =
 * unit(left_top + delta_x * (i as f32 / width as f32) + delta_y * (j as f32 / height as f32)) in f32 without FMA (viewport.rs:77-80, :63).
 * RTW_E_INVALID for a NULL pointer or a zero size. */
int rtw_depth_rays(const RtwCamera *cam, uint32_t width, uint32_t height, float *rays_out /* [height*width][6] */);
/* The closest hit of each of n_rays rays ([n][6] = origin, direction) within [mint, maxt]: t_out[i] = its t, idx_out[i] = its top-level
 * index; a miss writes +inf and -1.  normal_out ([n][3], may be NULL): the normal, 0 0 0 on a miss.  stats (may be NULL): segments
 * (= n_rays), sphere_tests, node_tests, quad_tests, kernel_ms.  rays, t_out, idx_out and normal_out may each be host memory or device
 * memory of ctx's GPU, as rtw_ctx_render's out_rgb (host memory is staged).  Blocking.  RTW_E_INVALID for a NULL ctx / rays / t_out /
 * idx_out, n_rays == 0 or an unknown accel; RTW_E_NO_SCENE before rtw_ctx_set_scene. */
int rtw_ctx_scene_hits(rtw_ctx *ctx, const float *rays, uint32_t n_rays, float time, float mint, float maxt, uint32_t accel,
                       float *t_out, int32_t *idx_out, float *normal_out, RtwStats *stats);
/* Viewport::depth_map in one launch: the kernel builds the ray of every pixel itself, by the rule of rtw_depth_rays, and writes
 * depth_out[j][i] = hit.t, or maxt * 1.6f on a miss (viewport.rs:68).  Row j of the output is row j of the image (the reference's
 * leading empty row, an artefact of `vec![vec![]]`, is not reproduced).  idx_out ([height][width], -1 on a miss) and normal_out
 * ([height][width][3]) may be NULL; memory kinds, stats and statuses as rtw_ctx_scene_hits (width * height must fit 32 bits). */
int rtw_ctx_depth_map(rtw_ctx *ctx, const RtwCamera *cam, uint32_t width, uint32_t height, float time, float mint, float maxt,
                      uint32_t accel, float *depth_out, int32_t *idx_out, float *normal_out, RtwStats *stats);

/* ---- surface buffers: the render's hit record of the first surface -- added within v4 ---------------------------------------------------
 * rtw_ctx_scene_hits with the rest of the winner's hit record: what the render's SHADE step reads of that hit under `integrator`, formed
 * once per ray, after the walk, by the functions the render kernels call.  t_out, idx_out and normal_out are rtw_ctx_scene_hits' answers
 * bit for bit -- ties, the tree-to-list equivalence under every fall-back, skipped constant-density instances, miss values.
 *   albedo_out   [n][3]  the colour the path's throughput is multiplied by: a sphere's texel * col_mod, a quad's or triangle's texel (or
 *                        their constant colours).  Under RTW_INTEGRATOR_RUST2, _LIGHT_CAST and _LIGHT_BIASED a textured sphere or triangle is
 *                        looked up by Rust2's rule (transposed index, scaled by the size) and `emitted` comes from RtwTexture.emit_tex.
 *   emitted_out  [n][3]  the emission of that hit (may be NULL)
 *   material_out [n][3]  metallicness, opacity, ir as the scene holds them; RTW_FLAG_MIXED_MATERIAL is the caller's to interpret (may be NULL)
 * An instance member, Euler or quaternion, is evaluated in the instance's frame, and a triangle of a placed mesh in the placement's.  A miss
 * writes 0 0 0 to all three.  Memory kinds, stats and stream order as rtw_ctx_scene_hits.  RTW_E_INVALID: everything rtw_ctx_scene_hits
 * refuses; albedo_out == NULL; an unknown integrator; NOT BUILT, also RTW_E_INVALID with nothing written: a context whose textures have
 * noise (rtw_ctx_set_texture_noise).  There is no rtw_mgpu_* form and no JSON form. */
int rtw_ctx_scene_surface(rtw_ctx *ctx, const float *rays, uint32_t n_rays, float time, float mint, float maxt, uint32_t accel,
                          uint32_t integrator, float *t_out, int32_t *idx_out, float *normal_out /* may be NULL */,
                          float *albedo_out /* [n][3] */, float *emitted_out /* [n][3], may be NULL */,
                          float *material_out /* [n][3] = metallicness, opacity, ir; may be NULL */, RtwStats *stats);
/* How rtw_ctx_surface_map makes the ray of pixel (i, j):
 *   RTW_RAYS_DEPTH_MAP  rtw_depth_rays' rule (cameras of rtw_camera2_new); offset is not read
 *   RTW_RAYS_PIXEL      for cameras of rtw_viewport_new: origin = cam.origin, direction = (pixel00 + delta_u * ((float)i + offset[0])) +
 *                       delta_v * ((float)j + offset[1]), not normalised.  Offset 0 0 is RTW_SAMPLER_NO_RAND's ray exactly; 0.5 0.5 is the
 *                       centre of the jittered samplers' pixel.  A NULL offset is 0 0. */
enum { RTW_RAYS_DEPTH_MAP = 0, RTW_RAYS_PIXEL = 1 };
/* Host only, pure: the rays of RTW_RAYS_PIXEL, f32 without FMA, row-major at rays_out[(j * width + i) * 6].  RTW_E_INVALID for a NULL cam
 * or rays_out or a zero size. */
int rtw_pixel_rays(const RtwCamera *cam, uint32_t width, uint32_t height, const float offset[2], float *rays_out /* [h*w][6] */);
/* What a camera sees: rtw_ctx_scene_surface over the rays of `ray_rule`, built in the kernel.  depth_out is t, or maxt * 1.6f on a miss as
 * rtw_ctx_depth_map writes it; with RTW_RAYS_DEPTH_MAP depth_out, idx_out and normal_out are rtw_ctx_depth_map's bytes; with RTW_RAYS_PIXEL
 * everything equals rtw_ctx_scene_surface over rtw_pixel_rays (but for that miss value).  idx_out, normal_out, emitted_out and
 * material_out may be NULL.  RTW_E_INVALID: everything rtw_ctx_depth_map and rtw_ctx_scene_surface refuse; an unknown ray_rule. */
int rtw_ctx_surface_map(rtw_ctx *ctx, const RtwCamera *cam, uint32_t width, uint32_t height, uint32_t ray_rule, const float offset[2],
                        float time, float mint, float maxt, uint32_t accel, uint32_t integrator,
                        float *depth_out, int32_t *idx_out, float *normal_out, float *albedo_out, float *emitted_out,
                        float *material_out, RtwStats *stats);

/* The surface calls with the triangle under each ray and the point's place inside it -- added within v4 (the calls above stay as they are).
 *   tri_out  [n] / [height][width] i32      a winner that is a world-space triangle or a triangle of a mesh placement: its position in the
 *                                           list rtw_ctx_set_triangles took, i.e. the row of `ouv`; every other winner and a miss: -1
 *   bary_out [n][2] / [height][width][2] f32   (alfa, beta) as the hit test forms them for that winner: p = o + d * t, planar = p - origin,
 *                                           alfa = w . (planar x v), beta = w . (u x planar), w = n / (n . n), n = u x v; for a placement
 *                                           (o, d) is the ray turned into the placement's frame; otherwise 0 0
 * Either may be NULL; with both NULL these are the calls above.  Everything else is written as by the calls above, byte for byte. */
int rtw_ctx_scene_surface_tri(rtw_ctx *ctx, const float *rays, uint32_t n_rays, float time, float mint, float maxt, uint32_t accel,
                              uint32_t integrator, float *t_out, int32_t *idx_out, float *normal_out, float *albedo_out, float *emitted_out,
                              float *material_out, int32_t *tri_out, float *bary_out, RtwStats *stats);
int rtw_ctx_surface_map_tri(rtw_ctx *ctx, const RtwCamera *cam, uint32_t width, uint32_t height, uint32_t ray_rule, const float offset[2],
                            float time, float mint, float maxt, uint32_t accel, uint32_t integrator, float *depth_out, int32_t *idx_out,
                            float *normal_out, float *albedo_out, float *emitted_out, float *material_out, int32_t *tri_out,
                            float *bary_out, RtwStats *stats);
/* Host only, pure: that rule from the mesh's ouv rows alone ([n_tris][9] = origin, u, v): for 0 <= tri[i] < n_tris the w of row tri[i] as
 * Triangle::new derives it and (alfa, beta) of ray i ([n][6]) at t[i]; any other tri[i]: 0 0, no address formed.  For a placed mesh pass the
 * rays of rtw_mesh_local_rays.  RTW_E_INVALID: a NULL pointer, n == 0, n_tris == 0. */
int rtw_tri_bary(const float *ouv, uint32_t n_tris, const float *rays, uint32_t n, const float *t, const int32_t *tri, float *bary_out);
/* Host only, pure: ray i as placement idx[i] - first meets it -- o' = qn.rotate(o - position), d' = qn.rotate(d), the walk's own operations
 * ("mesh placements" below); poses [n_mesh][7].  A ray whose idx names no placement, or a refused pose, is copied.  RTW_E_INVALID: a NULL
 * pointer, n == 0, n_mesh == 0 or beyond RTW_MAX_MESH_INSTANCES. */
int rtw_mesh_local_rays(const float *poses, uint32_t n_mesh, uint32_t first, const int32_t *idx, const float *rays, uint32_t n,
                        float *rays_out /* [n][6] */);

/* ---- light-biased integrators (Rust2/src/viewport/ray_color.rs:55-164, objects/material.rs material_pdf) ---------------------------
 * RTW_INTEGRATOR_LIGHT_CAST / RTW_INTEGRATOR_LIGHT_BIASED send, from every surface hit h, one shadow ray per light: towards the MID-POINT of
 * the light's bounding box (no random draw), `Ray::new(h.p, unit(mid - h.p))` with ray.time 0 whatever the path's time.  The light counts when
 * the closest hit of that ray over the whole scene IS the light (the same top-level object: the reference compares hit records, `hr.0 == hl`,
 * which differs from this only for coincident duplicate objects).  Then, with e the light's emitted colour at that hit (the constant, or for a
 * textured sphere Rust2's emission image, RtwTexture.emit_tex), pdf = material_pdf of the SURFACE's material for the shadow ray and
 * distance2 = t * t * |dir|^2:
 *   LIGHT_BIASED: skipped when pdf <= 1 / (255 * max(e.x, e.y, e.z)); else count += w, S += e * pdf / distance2 * w   (count starts at 1)
 *   LIGHT_CAST:   count += 1, S += e * pdf / distance2                                                               (count starts at 0)
 * and the hit returns (next + S) (.) multiplied / count + emmited (LIGHT_CAST: S (.) multiplied / count + emmited, emmited alone when count == 0),
 * evaluated front to back (DESIGN.md "Light-biased integrators" gives the association).  Materials as RTW_INTEGRATOR_RUST2 selects them:
 * opacity > 0 MirrorGlass, metallicness == 1 Mirror, else Lambertian.  Nothing is guarded that the reference does not guard: a hit point that is
 * the mid-point gives a NaN direction: the reference's sphere test ACCEPTS such a ray (every comparison with its NaN root is false) and reports
 * the first top-level sphere of the list, so when that sphere is the light a 0 or NaN pdf flows into S, and otherwise nothing is added; a light
 * that emits nothing gives 1 / 0 = inf as the skip threshold (LIGHT_BIASED always skips it).
 * The shadow rays draw nothing: the random stream of a LIGHT_BIASED path is RTW_INTEGRATOR_RUST2's, and with no lights set (or w == 0 and
 * finite terms) the image is RTW_INTEGRATOR_RUST2's bit for bit.  RtwStats.segments counts the shadow queries, camera_rays does not change.
 * A light names a TOP-LEVEL sphere or quad of the scene; lights inside instances and triangle lights are not expressible.
 * Renders with these integrators return RTW_E_UNSUPPORTED while triangles or texture noise are set, or when the scene holds a constant-density
 * instance (its hit draws ln(xi); Rust2 has no media).  Without a light list both integrators are legal (the loop is empty). */
#define RTW_MAX_LIGHTS 16u
enum { RTW_LIGHT_SPHERE = 0, RTW_LIGHT_QUAD = 1 };
typedef struct RtwLight {
    uint32_t kind;        /* RTW_LIGHT_SPHERE: RtwScene.spheres[index]; RTW_LIGHT_QUAD: RtwScene.quads[index] */
    uint32_t index;
} RtwLight;
/* The lights of the scene of the last rtw_ctx_set_scene (which clears them), and biased_weight (the reference's test uses 100).
 * lights == NULL with n == 0 clears them.  RTW_E_NO_SCENE before any scene; RTW_E_INVALID for n > RTW_MAX_LIGHTS, a NULL / n mismatch, an
 * unknown kind or an index beyond the scene, and while a render of the context is pending.  A sphere light's mid-point is formed from
 * RtwSphere.center alone -- its place at ray.time 0, the time of the shadow rays; the velocity is not read. */
int rtw_ctx_set_lights(rtw_ctx *ctx, const RtwLight *lights, uint32_t n, float biased_weight);
int rtw_mgpu_set_lights(rtw_mgpu *m, const RtwLight *lights, uint32_t n, float biased_weight);
/* Host only (no context, no GPU): the argument checks of rtw_ctx_set_lights for a light list against `scene`: RTW_OK or RTW_E_INVALID. */
int rtw_lights_validate(const RtwScene *scene, const RtwLight *lights, uint32_t n);
/* Host only, for tests and tools: the pure pieces, the same definitions the kernels compile (csrc/rtw_light.h).
 * rtw_light_mid: the mid-point (min + max) * 0.5 per axis of the light's box -- sphere: origin -/+ radius (Rust2/src/objects/sphere.rs:22-34);
 * quad: its four corners, an axis thinner than 0.005 widened to that about its centre first (objects/quad.rs:53-110).  RTW_E_INVALID as
 * rtw_ctx_set_lights. */
int rtw_light_mid(const RtwScene *scene, const RtwLight *light, float mid[3]);
/* material_pdf(h, r) (objects/material.rs:45-62, 93-99, 199-232) of the material mat3 = {metallicness, opacity, ir} for the hit
 * h = {p, n, incoming ray direction dir_in and time time_in} and the ray r = {ray_o, ray_d, ray_time}. */
float rtw_material_pdf(const float mat3[3], const float p[3], const float n[3], const float dir_in[3], float time_in,
                       const float ray_o[3], const float ray_d[3], float ray_time);
/* One accepted light of the loop above: updates S[3] and *count as `integrator` (LIGHT_CAST / LIGHT_BIASED) does for a light with emitted
 * colour e, hit at parameter t by the shadow ray of direction dir.  Returns 1 when the light was added, 0 when LIGHT_BIASED skipped it,
 * RTW_E_INVALID for another integrator or a NULL pointer. */
int rtw_light_term(uint32_t integrator, float pdf, const float e[3], float t, const float dir[3], float biased_weight, float S[3], float *count);

/* ---- MixedMaterial (Rust2/src/objects/material.rs:235-297, onb.rs:30-44) ----------------------------------------------------------
 * With RTW_FLAG_MIXED_MATERIAL, under RTW_INTEGRATOR_RUST2, RTW_INTEGRATOR_LIGHT_CAST and RTW_INTEGRATOR_LIGHT_BIASED, a sphere, quad or instance
 * member whose opacity < 0 is `MixedMaterial::new(exp)` with exp = ir (gen_exp = 1 / (exp + 1)); opacity > 0 stays MirrorGlass and opacity == 0
 * keeps its meaning (Mirror or Lambertian by metallicness).  Without the flag nothing changes: opacity < 0 is Mirror or Lambertian.
 *   on_hit: two draws from the pixel's stream, xi_phi then xi_cos;  phi = (xi_phi * 2) * PI, cos_theta = pow(1 - xi_cos, gen_exp),
 *     sin_theta = sqrt(1 - cos_theta^2), local = (cos(phi) sin_theta, sin(phi) sin_theta, cos_theta);  the basis is ONB::new_from_w(h.n):
 *     w = unit(n), a = (0,1,0) when |w.x| > 0.9 else (1,0,0), v = unit(w x a), u = unit(w x v);  direction = ((u x) + (v y)) + (w z).
 *     The normal is the hit's as reported, NOT flipped for a back-face hit (the lobe then points into the surface), and the scattered ray is
 *     built with Ray::new: its ray.time is 0, not the incoming ray's.
 *   material_pdf: 0 when the ray does not start at the hit point (1e-7 per component);  cos = unit(rd) . unit(n), negated unless din . n < 0;
 *     0 when cos < 0 (a NaN passes);  else pow(cos, exp) * (exp + 1) * (1 / 2 / PI).  No clamp at 1.
 * pow, sin and cos are the library's own total f32 functions (csrc/rtw_mixed.h: the same bits on host and device, 1.05 / 1.44 / 1.43 ulp at
 * most against f64 over the arguments a render can produce), where the reference calls the platform libm.
 * A render with the flag returns RTW_E_INVALID when a MixedMaterial object's exp is negative or not finite, and RTW_E_UNSUPPORTED when the scene
 * holds such an object together with triangles, texture noise or a constant-density instance.  MixedMaterial on triangles is not expressible.
 * With the flag set and no object with opacity < 0 in the scene the render is exactly the render without the flag. */
/* Host only (no context, no GPU): what a render of `scene` with `params` answers to the flag -- RTW_OK, RTW_E_UNSUPPORTED or RTW_E_INVALID as
 * above; n_triangles / texture_noise: as if that many triangles / any texture noise were set on the context. */
int rtw_mixed_validate(const RtwScene *scene, const RtwParams *params, uint32_t n_triangles, uint32_t texture_noise);
/* Host only, for tests and tools: the pure pieces, the same definitions the kernels compile (csrc/rtw_mixed.h).
 * rtw_mixed_dir: on_hit's direction for the two uniform draws.  rtw_mixed_pdf: material_pdf for the hit {p, n, incoming direction dir_in} and
 * the ray {ray_o, ray_d}. */
int rtw_mixed_dir(float exp, float xi_phi, float xi_cos, const float n[3], float out_dir[3]);
int rtw_mixed_pdf(float exp, const float p[3], const float n[3], const float dir_in[3], const float ray_o[3], const float ray_d[3], float *out);
/* The three elementary functions over arrays: out[i] = pow(x[i], y[i]) for x >= 0 (0, 1, inf, NaN included) and finite y >= 0 (libm's special
 * cases: pow(x, 0) = 1 even for a NaN x, pow(0, y > 0) = 0; x < 0 gives NaN); sin / cos of phi in [0, 2 pi] (NaN for NaN). */
int rtw_pow_plain(const float *x, const float *y, size_t n, float *out);
/* out[i] = exp(x[i]) for x <= 0 (csrc/rtw_exp.h, the guided filter's exponential): exp(+-0) = 1 exactly, exp(-inf) = 0, NaN for NaN, and a
 * result below 2^-126 is +0 (no subnormal is ever returned); x > 0 is outside the domain and gives NaN. */
int rtw_exp_plain(const float *x, size_t n, float *out);
int rtw_sin_plain(const float *phi, size_t n, float *out);
int rtw_cos_plain(const float *phi, size_t n, float *out);

/* ---- device math, for tests (csrc/rtw_probe.hip) -------------------------------------------------------------------------------------
 * The arithmetic sequences of the hot path (csrc/rtw_device.h, rtw_mixed.h, rtw_exp.h) evaluated directly on the GPU, the same definitions
 * the render, query and filter kernels compile.  Nothing here is needed to render.
 * rtw_ctx_device_math: out[i][0 .. out_cols) = fn(in[i][0 .. n_cols)) for i < n; element i is evaluated by thread i of a 1-D grid of
 * 256-thread blocks, so elements 64 w .. 64 w + 63 share a wave and a caller decides which path a wave-uniform range check takes.  in / out
 * are host memory (staged); n_cols / out_cols must be the function's (below), n >= 1.  On the context's stream, synchronised before it
 * returns; RTW_E_INVALID for a null pointer, n == 0, an unknown fn, wrong column counts, or while a render is pending.
 *   fn                        in                      out
 *   RTW_MATH_SQRT_PLAIN       x                       sqrt_plain(x)                       (meant for x in [2^-96, 2^127))
 *   RTW_MATH_SQRT_IEEE        x                       sqrt_ieee(x)
 *   RTW_MATH_DIV              n, d                    div_plain(n, d, rcp_refined(d))     (|d| in [2^-40, 2^40], |n| in [2^-60, 2^40] or 0)
 *   RTW_MATH_UNIT             x, y, z                 unit(a)  [3]
 *   RTW_MATH_UNIT_BALL        x, y, z, l2             unit_of_ball_point(p, l2)  [3]
 *   RTW_MATH_SPHERE_ROOT      b, disc, a, mint        sphere_root(b, disc, a, rcp_refined(a), a_plain, mint) with a_plain formed per wave as the
 *                                                     render kernels form it; NaN where disc < 0 (the kernels do not call it there)
 *   RTW_MATH_ATAN2            y, x                    atan2_plain(y, x)
 *   RTW_MATH_ACOS             x                       acos_plain(x)
 *   RTW_MATH_SPHERE_UV        x, y, z (a normal)      u, v  [2]
 *   RTW_MATH_LN               x                       ln_f32(x)
 *   RTW_MATH_POW              x, y                    pow_plain(x, y)
 *   RTW_MATH_SINCOS           phi                     sin, cos  [2]
 *   RTW_MATH_EXP              x                       exp_plain(x)
 * An argument outside a function's range gives a wrong number, never a fault. */
#define RTW_MATH_SQRT_PLAIN   0u
#define RTW_MATH_SQRT_IEEE    1u
#define RTW_MATH_DIV          2u
#define RTW_MATH_UNIT         3u
#define RTW_MATH_UNIT_BALL    4u
#define RTW_MATH_SPHERE_ROOT  5u
#define RTW_MATH_ATAN2        6u
#define RTW_MATH_ACOS         7u
#define RTW_MATH_SPHERE_UV    8u
#define RTW_MATH_LN           9u
#define RTW_MATH_POW         10u
#define RTW_MATH_SINCOS      11u
#define RTW_MATH_EXP         12u
#define RTW_MATH_COUNT       13u
int rtw_ctx_device_math(rtw_ctx *ctx, uint32_t fn, const float *in, uint32_t n_cols, uint32_t n, float *out, uint32_t out_cols);
/* rtw_ctx_device_sweep: argument sets too large to copy back.  Thread by thread the kernel forms the arguments of global index
 * first .. first + count - 1, evaluates the sequence and decides EXACTLY, in 64-bit integers, whether the result is the correctly rounded one.
 *   RTW_SWEEP_SQRT          sqrt_plain of the f32 whose bit pattern is the index (first + count <= 2^32; meant for 0x0F800000 .. 0x7F000000)
 *   RTW_SWEEP_DIV_RANDOM    div_plain_nz(n, d, rcp_refined(d)), which must also be div_plain's bits, of the pair a counter hash (lowbias32) of (seed, index) picks: independent signs,
 *                           24-bit mantissas, exponents uniform over |d| in [2^-40, 2^40) and |n| in [2^-60, 2^40)
 *   RTW_SWEEP_DIV_MIDPOINT  the same with mantissas whose exact quotient lies 1 / (2 md) < 2^-24 of an ulp from a rounding boundary, the
 *                           closest f32 operands allow: md an odd draw, c the odd 25-bit integer with c md = +-1 (mod 2^k), mn = (c md -+ 1) / 2^k
 *                           (the integer nearest to c md / 2^k), k = 24 or 25 so that mn has 24 bits
 * result: how many were tested, how many were wrong, and the first RTW_SWEEP_RECORDS wrong ones in the order the GPU met them -- the
 * arguments and the bits returned -- so that a failure can be read from the result alone.  count >= 1 and at most 2^32. */
#define RTW_SWEEP_SQRT          0u
#define RTW_SWEEP_DIV_RANDOM    1u
#define RTW_SWEEP_DIV_MIDPOINT  2u
#define RTW_SWEEP_COUNT         3u
#define RTW_SWEEP_RECORDS      16u
typedef struct RtwSweepResult {
    uint64_t tested, wrong;
    uint32_t n_records, reserved;                 /* min(wrong, RTW_SWEEP_RECORDS) */
    struct { uint32_t a, b, got, reserved; } records[RTW_SWEEP_RECORDS];   /* bit patterns: a = x or n, b = d (0 for sqrt), got = the result */
    float    kernel_ms;                           /* the sweep kernel alone, by HIP events */
    uint32_t reserved2;
} RtwSweepResult;
int rtw_ctx_device_sweep(rtw_ctx *ctx, uint32_t which, uint64_t first, uint64_t count, uint32_t seed, RtwSweepResult *result);
/* Host only: the sweeps' reference, so that it can itself be tested.  ok[i] = 1 when got[i] is the correctly rounded f32 result, else 0 (bit
 * patterns throughout).  RTW_SWEEP_SQRT: sqrt of a[i], b unused (may be null); a positive normal f32.  Otherwise got[i] against a[i] / b[i]:
 * a normal or a zero, b normal, and a right quotient that is normal or zero -- anything else is answered 0. */
int rtw_rounding_check(uint32_t which, const uint32_t *a, const uint32_t *b, const uint32_t *got, size_t n, uint8_t *ok);
/* Host only: the pairs a quotient sweep forms for indices first .. first + n - 1: out[i] = { n bits, d bits }. */
int rtw_sweep_operands(uint32_t which, uint64_t first, size_t n, uint32_t seed, uint32_t *out /* [n][2] */);

/* ---- quaternion-rotated instances (Rust2/src/objects/instance.rs:21-47, 215-255, quaternions.rs, rotation.rs) -------------------------
 * A Rust2 `Instance` carries a position and a QUATERNION rotation, where RtwInstance.rotation is Rust/'s Euler Vec3::rotated (another formula,
 * other bits).  With rotations set, an instance is hit as Rust2's Instance::get_hit writes it: r.origin -= position; r = r.rotated(q) (origin
 * and direction through Quaternion::rotate); the members are tested in that frame with the render's mint / maxt; the winner comes back as
 * p = q.rotate(p) + position, n = q.rotate(n) -- the SAME q both ways, not its conjugate (the reference's image depends on it); t is untouched.
 * The hit's ray (Rust2's Hit.r) is NOT turned back either: on_hit and material_pdf of a member read the direction in the instance's frame (the side
 * test of material_pdf is d_local . n, a Mirror reflects d_local about the turned normal), as the reference does.
 * Quaternion::rotate(v) = qn.hamilton((0, v)).hamilton(qn.conjugate()).get_vec(), qn = q * (1.0 / q.len()), len = sqrt(w*w + x*x + y*y + z*z);
 * hamilton as written (four products per component, added left to right), in f32 without FMA; the library forms qn once per instance on the
 * host with the same operations.  Members keep the library's order (the instance's spheres, then its quads).
 * rtw_ctx_set_instance_rotations: quat[i] = {w, x, y, z} for RtwScene.instances[i] of the last rtw_ctx_set_scene (which clears them); n must
 * equal the scene's instance count; quat == NULL with n == 0 clears them.  Every instance is then a quaternion instance -- (1, 0, 0, 0)
 * included, with no special case -- and ignores RtwInstance.rotation, which must be 0 there.  RTW_E_NO_SCENE before any scene; RTW_E_INVALID for
 * a count mismatch, a component that is not finite, a quaternion whose len is 0 or not finite, a non-zero Euler rotation or medium != 0 on an
 * instance (constant density is Rust/'s; the reference defines no mix of the two), and while a render of the context is pending.
 * Renders: RTW_INTEGRATOR_RUST2, _LIGHT_CAST and _LIGHT_BIASED, with or without RTW_FLAG_MIXED_MATERIAL, run the quaternion build of the render
 * kernels (shadow rays cross the rotated instances like any other ray).  NOT BUILT, RTW_E_INVALID at the render: any other integrator, active
 * texture noise, triangles in the context.  rtw_ctx_scene_hits / rtw_ctx_depth_map honour the rotations (the normal is q.rotate(n_local)).
 * The one-shot rtw_render / rtw_render_multi_gpu carry no rotations. */
int rtw_ctx_set_instance_rotations(rtw_ctx *ctx, const float (*quat)[4] /* w,x,y,z */, uint32_t n);
int rtw_mgpu_set_instance_rotations(rtw_mgpu *m, const float (*quat)[4], uint32_t n);
/* Host only (no context, no GPU): the argument checks of rtw_ctx_set_instance_rotations against `scene`: RTW_OK or RTW_E_INVALID. */
int rtw_instance_rotations_validate(const RtwScene *scene, const float (*quat)[4], uint32_t n);
/* Host only, pure, the same definitions the kernels compile (csrc/rtw_quat.h); quaternions are {w, x, y, z}.
 * rtw_quat_rotate: Quaternion::rotate (q need not be normalised).  rtw_quat_mul: a.hamilton(b) -- what Instance::rotate applies,
 * rotation = rotation.hamilton(rot).  rtw_quat_from_axis: Quaternion::new_from_axis(angle, axis): (cos(angle * 0.5), sin(angle * 0.5) *
 * unit(axis)) with the platform's sinf / cosf, as rtw_vec3_rotated uses them.  rtw_quat_from_euler: From<&EulerAngles> for euler = {x, y, z}.
 * RTW_E_INVALID for a NULL pointer. */
int rtw_quat_rotate(const float q[4], const float v[3], float out[3]);
int rtw_quat_mul(const float a[4], const float b[4], float out[4]);
int rtw_quat_from_axis(float angle, const float axis[3], float out[4]);
int rtw_quat_from_euler(const float euler[3], float out[4]);

/* ---- mesh placements: Rust2 instances of triangles (Rust2/src/objects/instance.rs:21-47, 215-255, triangle.rs) ---------------------------
 * A Rust2 `Instance` holds any Object, triangles included: a mesh is built once, translated, rotated and put into the scene several times.
 * Here the context's triangle mesh (rtw_ctx_set_triangles) is PLACED n times; placement k = {position, quat {w, x, y, z}}; all share one tree.
 * Replacement of the triangle group: with placements set the triangles are no longer a world-space group; the fourth group of the closest-hit
 * rule is the placements, tried in list order.
 * The test of placement k is Instance::get_hit: o' = q.rotate(o - position), d' = q.rotate(d) (Quaternion::rotate as in the section above; qn is
 * formed once per placement on the host with the same operations); the triangle group rule applies in that frame with the render's mint / maxt
 * (closest in list order, a later triangle only when strictly closer); t is untouched; the winner returns as p = q.rotate(p') + position,
 * n = q.rotate(n') -- the SAME q both ways, as for the quaternion instances.
 * Ordering: a later placement replaces an earlier one only when strictly closer; the group replaces the result so far (spheres, quads,
 * instances) only when strictly closer.
 * Hit.r stays local: under RTW_INTEGRATOR_RUST2 the material of a placed triangle reads the direction in the placement's frame -- a Mirror
 * reflects d' about the turned normal, MirrorGlass refracts d' -- and the next ray starts at the turned-back p.
 * Top-level index (rtw_ctx_scene_hits / rtw_ctx_depth_map): placement k reports n_spheres + n_quads + n_instances + k, normal q.rotate(n').
 * rtw_ctx_set_mesh_instances: rtw_ctx_set_scene and rtw_ctx_set_triangles clear the placements; NULL with n == 0 clears them; RTW_E_NO_SCENE
 * without triangles in the context; RTW_E_INVALID for n > RTW_MAX_MESH_INSTANCES, a NULL / n mismatch, a component that is not finite, a
 * quaternion whose len is 0 or not finite, any triangle with tex >= 0, and while a render is pending.  (Textured triangles: Triangle::color
 * reads alfa / beta from the turned-back h.p, triangle.rs:130-136, which for a member of a moved instance leaves [0, 1]; ImageTexture::color_at
 * then indexes outside the image -- a panic in the reference, so not expressible here.)
 * Renders: RTW_INTEGRATOR_RUST2 is served, with every sampler, flag and accel; everything the triangle build serves under that integrator next
 * to plain triangles stays legal next to placements.  NOT BUILT, RTW_E_INVALID at the render: every other integrator,
 * RTW_FLAG_MIXED_MATERIAL with a mixed object, instance rotations in the same context.  (Texture noise and lights are refused next to
 * triangles already.)  The one-shot rtw_render / rtw_render_multi_gpu carry no placements.  Without placements nothing changes.
 * The top-level tree (added within v4; Rust2 keeps its instances in an AABB tree, objects/aabb.rs:141-248): rtw_ctx_set_mesh_instances
 * builds a BVH over the placements' world boxes for every n >= 2 -- binned SAH, deterministic, nodes in the triangle tree's format, leaves
 * of up to 4 placements.  Placement k's box bounds conj(qn_k).rotate(x') + position_k over the mesh tree's root box -- where the geometry
 * stands for a ray; not the q.rotate(p') + position of the hit record, and not the reference's Instance::get_aabb, which turns the box the
 * wrong way -- padded for the rounding of the transform.  Under RTW_ACCEL_BVH a context with more than RTW_OPT_MESH_LIST_MAX placements
 * walks it and enters only placements whose box the ray meets.  The answer is the list order's ON THE BITS: the closest placement, of equal t
 * the lowest index, the group against the result so far only when strictly closer.  Where the bound's derivation does not hold the
 * placements are met in list order as before: a |position| or mesh extent beyond 2^38, a mesh whose own tree is refused, RTW_ACCEL_BRUTE, a
 * mint / maxt the triangle tree refuses; and per ray a non-finite component or |o|_inf + |d|_inf max(|mint|, |maxt|) > 2^38. */
typedef struct RtwMeshInstance { float position[3]; float quat[4]; /* w,x,y,z */ } RtwMeshInstance;
#define RTW_MAX_MESH_INSTANCES 65536u
int rtw_ctx_set_mesh_instances(rtw_ctx *ctx, const RtwMeshInstance *placements, uint32_t n);
int rtw_mgpu_set_mesh_instances(rtw_mgpu *m, const RtwMeshInstance *placements, uint32_t n);
/* Host only (no context, no GPU): the status rtw_ctx_set_mesh_instances answers for `placements` on a context that holds `tris`
 * (RTW_E_NO_SCENE for n_tris == 0). */
int rtw_mesh_instances_validate(const RtwTriangle *tris, uint32_t n_tris, const RtwMeshInstance *placements, uint32_t n);
/* Host only: the placement group by the list walk.  rays [n_rays][6] = origin, direction.  t_out: the hit's t, +inf on a miss;
 * placement_out / tri_out: the winning placement and its triangle (caller's list), -1 on a miss; normal_out ([n_rays][3], may be NULL):
 * q.rotate(n'), 0 on a miss.  RTW_E_INVALID for a NULL pointer, n_rays == 0, n == 0 or placements the validation refuses. */
int rtw_mesh_instance_hits(const RtwTriangle *tris, uint32_t n_tris, const RtwMeshInstance *placements, uint32_t n,
                           const float *rays, uint32_t n_rays, float mint, float maxt,
                           float *t_out, int32_t *placement_out, int32_t *tri_out, float *normal_out /* may be NULL */);
/* The same on the context's GPU through the function the render's closest-hit stage calls (host buffers in and out, blocking, as
 * rtw_ctx_triangle_hits): accel = RTW_ACCEL_BVH walks the mesh's tree in each placement it enters (rays the cull does not cover in a
 * placement's frame walk the list there) and reaches the placements through the top-level tree where the context has more than
 * RTW_OPT_MESH_LIST_MAX of them, else in list order; RTW_ACCEL_BRUTE walks the list of placements and in each the list of triangles.
 * stats (may be NULL): quad_tests = triangle tests, node_tests = node visits, the top-level tree's included.  RTW_E_NO_SCENE without placements. */
int rtw_ctx_mesh_instance_hits(rtw_ctx *ctx, const float *rays, uint32_t n_rays, float mint, float maxt, uint32_t accel,
                               float *t_out, int32_t *placement_out, int32_t *tri_out, float *normal_out /* may be NULL */, RtwStats *stats);
/* A node of the top-level tree (and of the triangle tree), depth-first: the left child of an inner node follows it, `skip` is the node after
 * its subtree (n_nodes: the end); leaf = (first << 3) | count names count <= 4 entries of the order array from `first`, 0: an inner node. */
typedef struct RtwTriNode { float lo[3]; uint32_t skip; float hi[3]; uint32_t leaf; } RtwTriNode;
/* Host only (added within v4): the top-level tree a context would build for `placements` of the mesh `tris`, as the device reads it.
 * nodes_out (may be NULL; node_cap entries, RTW_E_INVALID when too few -- 2 n - 1 always suffice: every leaf holds a placement, and SAH may
 * split one off per level; call with NULL first for the exact count) and *n_nodes; order_out ([n], may be NULL): the
 * placement indices in leaf order; *depth; *list_walk = 1: the context meets its placements in list order whatever the option says (a
 * placement or the mesh beyond the bound's reach, or the mesh's own tree refused).  Statuses as rtw_mesh_instance_hits. */
/* RTW_OPT_MESH_LIST_MAX as a new context holds it (host only; added within v4). */
uint32_t rtw_mesh_list_max_default(void);
int rtw_mesh_top_dump(const RtwTriangle *tris, uint32_t n_tris, const RtwMeshInstance *placements, uint32_t n,
                      RtwTriNode *nodes_out, uint32_t node_cap, uint32_t *n_nodes, uint32_t *order_out, uint32_t *depth, uint32_t *list_walk);
/* Host only (added within v4): rtw_mesh_instance_hits' arguments and outputs through the walk the kernels run under RTW_ACCEL_BVH with
 * RTW_OPT_MESH_LIST_MAX = 0 -- the same source, compiled for the host: the top-level tree, in each entered placement the mesh's tree.  The
 * same bits as rtw_mesh_instance_hits.  stats (may be NULL): node_tests = node visits of both trees, quad_tests = triangle tests. */
int rtw_mesh_instance_hits_tree(const RtwTriangle *tris, uint32_t n_tris, const RtwMeshInstance *placements, uint32_t n,
                                const float *rays, uint32_t n_rays, float mint, float maxt,
                                float *t_out, int32_t *placement_out, int32_t *tri_out, float *normal_out /* may be NULL */, RtwStats *stats);

/* ---- refit: a deforming mesh (added within v4) -------------------------------------------------------------------------
 * The triangles of rtw_ctx_set_triangles move; the tree keeps its topology.  ouv: [n][9] f32 = origin, u, v of every triangle in the
 * caller's list order, n the context's triangle count; a device or managed pointer of the context's GPU is read in place, anything else is
 * staged.  On the device, on the context's stream (rtw_ctx_set_stream: behind the caller's producers of `ouv`), every triangle's derived
 * fields are recomputed (Triangle::new) and every box of the tree from its triangles, inflated and rounded outward as the builder does.
 * Materials, `tex`, the leaf order and the skip links stay.  The tree only prunes and every candidate runs the exact test, so a render or
 * query after a refit gives what rtw_ctx_set_triangles of the same triangles gives, bit for bit; what a refit may cost is node visits (the
 * splits were chosen for the old shape).  rtw_ctx_set_triangles remains the way to rebuild.  The call ends with one stream synchronise;
 * *list_walk_out (may be NULL) = 1 when a triangle now breaks a condition of the tree (rtw_ctx_set_triangles' list) and the context walks
 * the list until a later refit or set brings 0.  It reserves no memory.  RTW_E_NO_SCENE without triangles; RTW_E_INVALID for a NULL
 * pointer, n other than the context's count, a pending render, and while placements are set (their top-level tree was built over the old
 * root box: rtw_ctx_move_mesh_instances refits both).  After RTW_E_HIP the triangles may be partly moved: placements are refused until a refit
 * or rtw_ctx_set_triangles succeeds.  No rtw_mgpu_* form. */
int rtw_ctx_refit_triangles(rtw_ctx *ctx, const float *ouv, uint32_t n, uint32_t *list_walk_out);
/* The nodes of the context's triangle tree as the device holds them now.  nodes_out (may be NULL; node_cap entries, RTW_E_INVALID when too
 * few) and *n_nodes (may be NULL).  RTW_E_NO_SCENE without triangles. */
int rtw_ctx_triangle_bvh_dump(rtw_ctx *ctx, RtwTriNode *nodes_out, uint32_t node_cap, uint32_t *n_nodes);
/* Host only: the tree rtw_ctx_set_triangles builds for `tris` -- nodes_out / node_cap / *n_nodes as above (2 n - 1 always suffice);
 * order_out ([n], may be NULL): the triangle indices in leaf order; *depth; *list_walk.  RTW_E_INVALID for no triangles. */
int rtw_triangle_bvh_dump(const RtwTriangle *tris, uint32_t n, RtwTriNode *nodes_out, uint32_t node_cap, uint32_t *n_nodes,
                          uint32_t *order_out, uint32_t *depth, uint32_t *list_walk);
/* Host only: that tree after a refit to `ouv` ([n][9]) -- the functions and the schedule the device runs, compiled for the host: the bytes
 * rtw_ctx_triangle_bvh_dump returns after rtw_ctx_refit_triangles(ouv).  *list_walk as rtw_ctx_refit_triangles gives it. */
int rtw_triangle_bvh_refit(const RtwTriangle *tris, uint32_t n, const float *ouv, RtwTriNode *nodes_out, uint32_t node_cap,
                           uint32_t *n_nodes, uint32_t *list_walk);

/* ---- moving placements (added within v4) -----------------------------------------------------------------------------------
 * The placements of rtw_ctx_set_mesh_instances take new poses and / or the mesh new triangles; both trees keep their topology.
 * poses: [n][7] f32 = position xyz, quat wxyz (the layout of RtwMeshInstance), n = the context's placement count, or NULL: the poses stay.
 * ouv:   [n_tris][9] f32 as rtw_ctx_refit_triangles takes it, or NULL: the mesh stays.  Not both NULL.  A device or managed pointer of the
 * context's GPU is read in place, anything else is staged into memory the setters reserved: the call reserves none.  On the context's
 * stream, behind the caller's producers: the triangle refit (ouv given), then one thread per leaf of the top-level tree forms the rows of
 * its placements and their world boxes from the mesh's root box as the device holds it, then the inner boxes bottom-up; one stream
 * synchronise at the end.  The tree only prunes and the winner among placements is the least (t, index) in any visiting order, so a render
 * or query afterwards gives what rtw_ctx_set_triangles + rtw_ctx_set_mesh_instances of the moved mesh and poses give, bit for bit; a moved
 * tree may cost node visits, rtw_ctx_set_mesh_instances rebuilds.
 * An INVALID pose (a component that is not finite, a quaternion whose len is 0 or not finite -- decided on the device, for host and device
 * input alike) leaves its placement where it was; every other placement moves, the context is consistent (it holds the list with the bad
 * entries replaced by their old poses) and the call returns RTW_E_INVALID.
 * *list_walk_out (may be NULL; also written with that RTW_E_INVALID): bit 0 = a triangle breaks a condition of the mesh's tree
 * (rtw_ctx_refit_triangles' answer); bit 1 = a placement or the mesh lies beyond 2^38 and the placements are met in list order until a later
 * move brings 0 (rtw_ctx_set_mesh_instances keeps the tree in that case too, so that a move can recover it).
 * RTW_E_NO_SCENE without placements; RTW_E_INVALID for both pointers NULL, n / n_tris other than the context's counts for a given pointer, a
 * pending render, and a stale mesh root (rtw_ctx_refit_triangles) with ouv == NULL.  After RTW_E_HIP neither tree is walked and the root is
 * stale, as after a refit that stopped.  No rtw_mgpu_* form. */
int rtw_ctx_move_mesh_instances(rtw_ctx *ctx, const float *poses, uint32_t n, const float *ouv, uint32_t n_tris, uint32_t *list_walk_out);
/* The context's top-level tree and placement rows as the device holds them now: nodes_out (may be NULL; node_cap entries, RTW_E_INVALID when
 * too few) and *n_nodes (may be NULL; one leaf for a single placement); rows_out ([n][8] f32, may be NULL): per placement the normalised
 * quaternion w, x, y, z, then position, 0.  RTW_E_NO_SCENE without placements. */
int rtw_ctx_mesh_top_dump(rtw_ctx *ctx, RtwTriNode *nodes_out, uint32_t node_cap, uint32_t *n_nodes, float *rows_out /* [n][8], may be NULL */);
/* Host only: the top-level tree built for `placements`, refitted to `moved` ([n][7], may be NULL) with the mesh refitted to `ouv` (may be
 * NULL) -- the functions and the schedules the device runs, compiled for the host: the bytes rtw_ctx_mesh_top_dump returns after
 * rtw_ctx_set_mesh_instances(placements) and rtw_ctx_move_mesh_instances(moved, ouv).  *list_walk as the move gives it; *n_invalid: the
 * invalid poses of `moved` (the status stays RTW_OK: their placements keep their rows).  Statuses as rtw_mesh_top_dump. */
int rtw_mesh_top_refit(const RtwTriangle *tris, uint32_t n_tris, const RtwMeshInstance *placements, uint32_t n, const float *moved /* [n][7] */,
                       const float *ouv, RtwTriNode *nodes_out, uint32_t node_cap, uint32_t *n_nodes, float *rows_out /* [n][8], may be NULL */,
                       uint32_t *list_walk, uint32_t *n_invalid);

/* ---- occlusion queries: any-hit over the whole scene (added within v4) -------------------------------------------------
 * "Is anything in the way?" for shadow tests, line of sight, visibility masks and ambient occlusion: one byte per ray, with the early exit a
 * closest-hit query cannot take.  THE CONTRACT: occluded_out[i] == 1 exactly when rtw_ctx_scene_hits with the same rays, time, mint, maxt and
 * accel reports an index >= 0 for ray i, else 0 -- for every ray (NaN rays, zero directions, the rays the trees refuse, a root exactly at
 * mint or maxt, mint > maxt), under both accels and every fall-back to the lists, RTW_OPT_LIST_WALK_MAX and RTW_OPT_MESH_LIST_MAX honoured as
 * there.  It is exact, not approximate: every group's acceptance of a candidate with nothing found so far depends on the candidate and on
 * [mint, maxt] alone, and the trees only prune.  Constant-density instances are skipped, the direction is used as given (t in units of |d|),
 * every group is served (spheres, quads, instances with either rotation, triangles, mesh placements), and a refit or a move is seen by the
 * next query.  A lane stops at its first accepted candidate, so every counter is <= rtw_ctx_scene_hits' on the same rays.
 * rays ([n_rays][6] = origin, direction) and occluded_out ([n_rays] bytes) may each be host memory or device memory of ctx's GPU (host memory
 * is staged); the work runs on the stream of rtw_ctx_set_stream; blocking.  stats (may be NULL): segments (= n_rays), sphere_tests,
 * node_tests, quad_tests, kernel_ms.  RTW_E_INVALID for a NULL ctx / rays / occluded_out, n_rays == 0 or an unknown accel; RTW_E_NO_SCENE
 * before rtw_ctx_set_scene.  No per-ray ranges and no rtw_mgpu_* form (the camera form is rtw_ctx_ao_map, below). */
int rtw_ctx_scene_occluded(rtw_ctx *ctx, const float *rays, uint32_t n_rays, float time, float mint, float maxt,
                           uint32_t accel, uint8_t *occluded_out, RtwStats *stats);
/* Host only: the kernel's triangle group and placement group, the same source compiled for the host -- the mesh's tree where the device would
 * take it under RTW_ACCEL_BVH, the top-level tree as under RTW_OPT_MESH_LIST_MAX = 0, the lists otherwise.  occluded_out[i] == 1 exactly when
 * rtw_triangle_hits / rtw_mesh_instance_hits reports an index >= 0.  stats (may be NULL): segments, node_tests = node visits of both trees,
 * quad_tests = triangle tests.  Statuses as rtw_triangle_hits / rtw_mesh_instance_hits.  (The library has no CPU path for spheres, quads or
 * instances, so there is no host form of the whole query.) */
int rtw_triangle_occluded(const RtwTriangle *tris, uint32_t n, const float *rays, uint32_t n_rays, float mint, float maxt,
                          uint8_t *occluded_out, RtwStats *stats);
int rtw_mesh_instance_occluded(const RtwTriangle *tris, uint32_t n, const RtwMeshInstance *placements, uint32_t n_placements,
                               const float *rays, uint32_t n_rays, float mint, float maxt, uint8_t *occluded_out, RtwStats *stats);

/* ---- ambient occlusion: hemisphere any-hit rays, fused (added within v4) ------------------------------------------------
 * For each point, `samples` cosine-weighted rays about its normal, walked by the any-hit pass in the kernel that makes them, one float out:
 * the share of the rays that nothing stops within [mint, maxt] (maxt is the AO radius: the directions are unit to rounding).  No ray is
 * stored anywhere.
 * THE RULE (rtw_ao_rays; csrc/rtw_ao.h): ray [i][k] of point i, sample k under `seed` has the origin points[i] as given (no bias: mint keeps
 * the ray off its own surface) and the direction rtw_mixed_dir(1.0, xi_phi, xi_cos, normals[i]) -- exp = 1 is the cosine lobe --, where
 * xi_phi, xi_cos are the first two draws of the render's counter-based stream started at sample k of
 * base = mix32(mix32(mix32(seed + 0x9E3779B9) ^ 0x414F5241) ^ i).  Ray [i][k] depends on (seed, i, k, point, normal) alone: not on n, not
 * on samples.  A point whose normal is exactly (0, 0, 0) is SKIPPED: it casts no rays and answers 1.0 (rtw_ctx_depth_map's miss pixels have
 * this normal); rtw_ao_rays writes six zeros for each of its rays.  Everything else flows: a NaN point or normal gives NaN rays.
 * THE CONTRACT: for a point that is not skipped, ao_out[i] == (float)(samples - c_i) * (1.0f / samples), c_i the number of k < samples for
 * which rtw_ctx_scene_occluded answers 1 for ray [i][k] of rtw_ao_rays with the same time, mint, maxt and accel -- exactly, for every input,
 * under both accels and every fall-back: an any-hit answer depends on the ray alone, never on the lanes that share its wave.  samples must be
 * a power of two in 1 .. 1024, so the product is exact.
 * points, normals ([n][3]) and ao_out ([n]) may each be host memory or device memory of ctx's GPU (host memory is staged); the work runs on
 * the stream of rtw_ctx_set_stream; blocking.  stats (may be NULL): segments = the rays cast (samples x the points not skipped),
 * sphere_tests, node_tests, quad_tests = rtw_ctx_scene_occluded's on those rays, kernel_ms.  RTW_E_INVALID for a NULL ctx / points /
 * normals / ao_out, n == 0, a samples that is not a power of two in 1 .. 1024, n x samples above 2^32 - 1, an unknown accel or a call while
 * a render is pending; RTW_E_NO_SCENE before rtw_ctx_set_scene.  No bent normals, no per-point radii and no rtw_mgpu_* form. */
/* host only, pure */
int rtw_ao_rays(const float *points, const float *normals, uint32_t n, uint32_t samples, uint32_t seed,
                float *rays_out /* [n][samples][6]; six zeros for every ray of a skipped point */);
int rtw_ctx_ambient_occlusion(rtw_ctx *ctx, const float *points /*[n][3]*/, const float *normals /*[n][3]*/, uint32_t n,
                              uint32_t samples, uint32_t seed, float time, float mint, float maxt, uint32_t accel,
                              float *ao_out /*[n]*/, RtwStats *stats);
/* The camera form, defined as a composition: rtw_ctx_depth_map(cam, width, height, time, mint, maxt, accel) with ids and normals, then
 * rtw_ctx_ambient_occlusion over [ao_mint, ao_maxt] with point index j * width + i, the points p = o + d * depth for idx >= 0 (o, d by the
 * rule of rtw_depth_rays; one f32 rounding per operation, no FMA), the normals faced towards the viewer (dot(d, n) > 0 ? -n : n), a miss
 * pixel (idx < 0) skipped.  depth_out, idx_out and normal_out (each may be NULL) receive exactly rtw_ctx_depth_map's bytes -- the normal as
 * that call writes it, not faced.  Two launches between one pair of events: stats adds the depth pass's counters and its width x height
 * rays to the AO's.  Memory kinds, stream and blocking as above; RTW_E_INVALID also for a NULL cam, a zero width or height, or
 * width x height x samples above 2^32 - 1. */
int rtw_ctx_ao_map(rtw_ctx *ctx, const RtwCamera *cam, uint32_t width, uint32_t height, float time, float mint, float maxt,
                   uint32_t samples, uint32_t seed, float ao_mint, float ao_maxt, uint32_t accel,
                   float *ao_out /*[h][w]*/, float *depth_out, int32_t *idx_out, float *normal_out /* each may be NULL */,
                   RtwStats *stats);

/* ---- direct lighting: area-light shadow rays, fused (added within v4) --------------------------------------------------
 * "How much of each light does this point see?"  For every (point, light) pair -- the lights of rtw_ctx_set_lights --, `samples` any-hit
 * segments from the point to points sampled on the light's surface, walked in the kernel that makes them, two floats out: vis, the share of
 * the samples that are cast and reach the light, and irr, the mean of their geometric terms (an estimate of the irradiance for unit
 * radiance; neither the emitted colour nor 1 / pi is applied -- the caller multiplies).  No ray is stored anywhere.
 * THE RULE (rtw_light_samples; csrc/rtw_direct.h; f32, one rounding per written operation, no FMA).  Item (i, l) is point i under light l of
 * the list; xi1, xi2 are the first two draws of the render's counter-based stream started at sample k of
 * base = mix32(mix32(mix32(mix32(seed + 0x9E3779B9) ^ 0x4C495445) ^ i) ^ (l + 1)).
 *   quad light (RtwQuad origin o, edges u, v):  y = (o + u * xi1) + v * xi2
 *   sphere light (c = RtwSphere.center, its place at time 0 as rtw_light_mid reads it; radius r):  z = 1 - 2 * xi1, s = sqrt(1 - z * z),
 *     phi = 6.2831855f * xi2, w = (s * cos_plain(phi), s * sin_plain(phi), z), w = -w when dot(w, p - c) < 0, y = c + w * r
 * The ray has the origin p as given and the direction d = y - p, NOT normalised, and is walked over [lo, hi] in units of the segment
 * (1e-3 and 1 - 1e-3 leave out both end points' own surfaces: the light itself at t = 1 lies outside the range).  A sphere light hides the
 * part of its facing hemisphere beyond its own horizon: those samples are blocked by the light's near side and count as blocked.
 * A sample is CAST when the normal is not exactly (0, 0, 0) and dot(n, d) > 0 (a NaN fails); a sample that is not cast walks nothing and
 * counts nothing.  Its weight, with dd = dot(d, d) and the normal as given (a unit normal gives the geometric term):
 *   quad:    G = (dot(n, d) * fabs(dot(cross(u, v), d))) / (dd * dd)                     (the quad emits to both sides)
 *   sphere:  G = ((dot(n, d) * cl) * (6.2831855f * (r * r))) / (dd * dd),  cl = -dot(w, d) > 0 ? -dot(w, d) : 0
 * Ray [i][l][k] depends on (seed, i, l, k, point, normal, the light's geometry) alone: not on n, samples or the number of lights.
 * OUTPUTS: vis[i][l] = (float)v * (1.0f / samples), v the cast samples that nothing stops; irr[i][l] = S * (1.0f / samples), S the sum of
 * w_k (G_k for a cast and free sample, +0 otherwise) in this association: with L = min(samples, 64), s_g = ((0 + w_g) + w_{g+L}) + ... for
 * g < L, then s_g = s_g + s_{g+off} for g < off, off = L/2, L/4, ..., 1, S = s_0 (rtw_light_reduce).  samples: a power of two in 1 .. 1024.
 * THE CONTRACT: v is the number of cast k for which rtw_ctx_scene_occluded answers 0 for ray [i][l][k] of rtw_light_samples with the same
 * time, mint = lo, maxt = hi and accel -- exactly, for every input, under both accels and every fall-back --, and irr is rtw_light_reduce
 * of rtw_light_samples' weights with the blocked ones set to +0, bit for bit. */
/* host only, pure: the light list is checked as rtw_lights_validate checks it (an empty list is refused as well); RTW_E_INVALID also for a
 * NULL pointer, n == 0 or a samples that is not a power of two in 1 .. 1024.  A sample that is not cast gets six zeros and the weight 0. */
int rtw_light_samples(const RtwScene *scene, const RtwLight *lights, uint32_t n_lights, const float *points /*[n][3]*/,
                      const float *normals /*[n][3]*/, uint32_t n, uint32_t samples, uint32_t seed,
                      float *rays_out /*[n][n_lights][samples][6]*/, float *weight_out /*[n][n_lights][samples]*/);
/* host only, pure: *out = S * (1.0f / samples) of weights[0 .. samples) in the association above */
int rtw_light_reduce(const float *weights, uint32_t samples, float *out);
/* n_lights of the two calls below: the lights of the last rtw_ctx_set_lights (0: none set, or a NULL ctx) -- what sizes their outputs */
uint32_t rtw_ctx_light_count(const rtw_ctx *ctx);
/* points, normals ([n][3]), vis_out and irr_out ([n][n_lights]; irr_out may be NULL) may each be host memory or device memory of ctx's GPU
 * (host memory is staged); the work runs on the stream of rtw_ctx_set_stream; blocking.  stats (may be NULL): segments = the rays cast,
 * sphere_tests, node_tests, quad_tests = rtw_ctx_scene_occluded's over exactly those rays, kernel_ms.  RTW_E_INVALID for a NULL ctx /
 * points / normals / vis_out, n == 0, a samples that is not a power of two in 1 .. 1024, an unknown accel, a call while a render is
 * pending, no lights set, or n x n_lights x samples above 2^32 - 1; RTW_E_NO_SCENE before rtw_ctx_set_scene.  An invalid call writes
 * nothing.  No per-light sample counts, no emission or textures applied, no triangle lights and no rtw_mgpu_* form. */
int rtw_ctx_direct_light(rtw_ctx *ctx, const float *points /*[n][3]*/, const float *normals /*[n][3]*/, uint32_t n, uint32_t samples,
                         uint32_t seed, float time, float lo, float hi, uint32_t accel, float *vis_out /*[n][n_lights]*/,
                         float *irr_out /*[n][n_lights], may be NULL*/, RtwStats *stats);
/* The camera form, defined as a composition exactly as rtw_ctx_ao_map is: rtw_ctx_depth_map(cam, width, height, time, mint, maxt, accel)
 * with ids and normals, then rtw_ctx_direct_light over [lo, hi] with point index j * width + i, the points p = o + d * depth for idx >= 0,
 * the normals faced towards the viewer, a miss pixel skipped (its normal is 0 0 0: vis and irr 0).  depth_out, idx_out and normal_out
 * (each may be NULL) receive exactly rtw_ctx_depth_map's bytes.  Two launches between one pair of events: stats adds the depth pass's
 * counters and its width x height rays.  RTW_E_INVALID also for a NULL cam, a zero width or height, or
 * width x height x n_lights x samples above 2^32 - 1. */
int rtw_ctx_direct_light_map(rtw_ctx *ctx, const RtwCamera *cam, uint32_t width, uint32_t height, float time, float mint, float maxt,
                             uint32_t samples, uint32_t seed, float lo, float hi, uint32_t accel,
                             float *vis_out /*[h][w][n_lights]*/, float *irr_out, float *depth_out, int32_t *idx_out,
                             float *normal_out /* each but vis_out may be NULL */, RtwStats *stats);

/* ---- host mirror of the reference constructors (same library, no GPU needed) ---------------- */

/* Viewport::new (viewport.rs:308-401).  Options the reference takes as Option<> are pointers
 * (NULL == None).  Writes the camera and the derived height `(width as f32 / aspect) as u64`. */
int rtw_viewport_new(uint32_t width, float aspect_ratio, const float *vfov, const float *origin,
                     const float *direction, const float *vup, const float *lens_radius,
                     RtwCamera *cam, uint32_t *height);
/* Viewport::new_from_res (viewport.rs:402-428): aspect = width as f32 / height as f32. */
int rtw_viewport_new_from_res(uint32_t width, uint32_t height, const float *vfov, const float *origin,
                              const float *direction, const float *vup, const float *lens_radius,
                              RtwCamera *cam, uint32_t *height_out);
/* Rust2 `Camera::new(aspect, origin, vup, dir, vfov, lens_radius)` (Rust2/src/viewport/camera.rs:19-53) for
 * RTW_SAMPLER_CENTRES: pixel00 = left_top, delta_u/delta_v = the FULL-viewport delta_x/delta_y (divided by
 * width/height at use, Rust2/src/viewport.rs:95-99); the lens offset is the raw disk point (viewport.rs:101). */
int rtw_camera2_new(float aspect, const float origin[3], const float vup[3], const float dir[3], float vfov,
                    float lens_radius, RtwCamera *cam);
/* Sphere::new / new_moving (sphere.rs:151-199): col_mod==NULL -> (1,1,1); mat==NULL -> EMPTY_M. */
int rtw_sphere_new(const float origin[3], float radius, const float *col_mod,
                   const float *mat3 /* metallicness, opacity, ir */, const float *velocity,
                   RtwSphere *out);
/* Sphere::new_with_texture (sphere.rs:200-224). */
int rtw_sphere_new_with_texture(const float origin[3], float radius, const float *col_mod,
                                const float *mat3, const float *velocity, int32_t tex, RtwSphere *out);
/* Quad::new (quad.rs:84-110) with ImageTexture::from_color(color): velocity == NULL -> 0, emitted == NULL -> 0. */
int rtw_quad_new(const float origin[3], const float u[3], const float v[3], const float *mat3,
                 const float *emitted, const float color[3], RtwQuad *out);
/* Instance::new_box(a, b, tex, mat) (instance.rs:83-176): the six quads of the axis-aligned box, in the
 * reference's order, written to quads6[0..6). */
int rtw_box_quads(const float a[3], const float b[3], const float *mat3, const float color[3], RtwQuad quads6[6]);
/* Vec3::rotated(rot) (Rust/src/vec3.rs:161-181) as the library applies it to instances: sin / cos of the three angles on the
 * host, the products in the reference's written order (including its non-orthogonal terms for rotations about more than
 * one axis). */
void rtw_vec3_rotated(const float v[3], const float rot[3], float out[3]);
/* The tile permutation RTW_OPT_TILE_ORDER = mode uses for a whole width x height frame of this camera (host only; for tests and
 * tools): order[q] = index (row-major over the ceil(width/8) x ceil(height/8) tiles) of the tile the queue hands out q-th. */
int rtw_tile_order(uint32_t mode, uint32_t width, uint32_t height, const RtwCamera *cam, const RtwScene *scene,
                   uint32_t *order, uint32_t cap);
/* Rows a partition owns (see RtwParams). */
uint32_t rtw_part_rows(uint32_t height, uint32_t row_block, uint32_t part_index, uint32_t part_count);
/* write_img_f32 quantisation: round(clamp(c*255, 0, 255)) (Rust/src/write_img.rs:11-15). */
void rtw_quantize_u8(const float *rgb, size_t n_values, uint8_t *out);
/* Rust2 Vec3::to_rgb_u8: round(clamp(c*255.99, 0, 255)) (Rust2/src/vec3.rs:240-246). */
void rtw_quantize_u8_rust2(const float *rgb, size_t n_values, uint8_t *out);

/* ---- scene wire format and image writers (rtw_io.cpp; host only) -------------------------------- */
/* The reference's `json` scene object {"spheres":[{origin,radius,col_mod,material{metallicness,opacity,ir},
 * velocity,texture{row,col,img[]}}]} (Rust/src/viewport.rs:174-205, objects/sphere.rs:44-90,
 * objects/materials.rs:21-54, texture.rs:28-59; the C++ dialect without velocity/texture is accepted).
 * rtw_scene_to_json returns the length needed; rtw_scene_from_json uses the count-query pattern
 * (spheres == NULL -> sizes only). */
size_t rtw_scene_to_json(const RtwScene *scene, char *buf, size_t cap);
int rtw_scene_from_json(const char *text, size_t len,
                        RtwSphere *spheres, uint32_t sphere_cap, uint32_t *n_spheres,
                        RtwTexture *textures, uint32_t texture_cap, uint32_t *n_textures,
                        float *texels, uint32_t texel_cap, uint32_t *n_texels);
/* write_img_f32 (Rust/src/write_img.rs:6-19): quantise and save an 8-bit RGB PNG. */
int rtw_write_png_f32(const char *path, const float *rgb, uint32_t width, uint32_t height);
/* write_ppm (C++/src/ppm_writer.cpp:12-27): P3 text with the C++ truncation int(255 c). */
int rtw_write_ppm_f32(const char *path, const float *rgb, uint32_t width, uint32_t height);

/* Host-side self-check of the acceleration structure rtw_ctx_set_scene would build (no GPU): every sphere is
 * reachable exactly once (tree leaf or big list), nested bounds, time-expanded for [t_begin, t_end], the f16 copy
 * contains the f32 boxes, depth within the device stack.  RTW_OK or RTW_E_INVALID; optional outputs describe the tree. */
int rtw_bvh_validate(const RtwScene *scene, float t_begin, float t_end,
                     uint32_t *n_nodes, uint32_t *depth, uint32_t *n_big, uint32_t *has_f16);
/* Testing and measuring entry points, not part of the render path: the CPU tests and the builder's yardstick read the tree through them.
 * The same tree, handed out (no GPU): `nodes` receives n_nodes 64-byte records {lo0[3], hi0[3], lo1[3], hi1[3], c0, c1, pad[2]} with
 * nodes[0] the root (child >= 0: node, < 0: ~sphere), `nodes16` (optional) the 32-byte f16 records when the tree has them, `big` the
 * spheres kept outside the tree; depth_cap is the depth the builder allowed itself.  Every output pointer may be NULL. */
int rtw_bvh_dump(const RtwScene *scene, float t_begin, float t_end, void *nodes, uint32_t node_cap, uint32_t *n_nodes, int32_t *root,
                 uint32_t *depth, uint32_t *depth_cap, uint32_t *big, uint32_t big_cap, uint32_t *n_big, uint16_t *nodes16);
/* The f32 plane format of those f16 nodes, as the large-workgroup builds of the render kernel hold a tree in LDS (RTW_OPT_NODE_FORMAT): every
 * plane widened exactly, laid out so that a ray reads {near, far} of a (box, axis) at a per-ray offset.  out: n_nodes * layout[0] dwords (may
 * be NULL: layout only); layout[4] = dwords per node, dwords per (box, axis) group, the byte offset at which a ray along +axis reads its
 * pair (a ray along -axis reads at 0), the code of an inner child per node index.  After the six groups: the dword {c0, c1} of 16-bit child codes
 * at both read offsets of the x group, each followed by the same two codes swapped, {c1, c0}.  A testing tool, no GPU. */
int rtw_bvh_pack_nodes32(const uint16_t *nodes16, uint32_t n_nodes, uint32_t *out, uint32_t out_cap, uint32_t *layout);
/* Host twin of the render kernel's closest-hit query over that tree (a measuring and testing tool, no GPU): rays = n x {origin[3],
 * direction[3]}; hit[i] = sphere index or -1, t[i] its parameter, visits[i] (optional) the inner-node visits, counted as
 * RtwStats.node_tests counts them.  use_tree == 0 walks the sphere list with the same sphere test.  The tree is built once per CALL:
 * pass the rays of a scene in one batch. */
int rtw_bvh_query_host(const RtwScene *scene, float t_begin, float t_end, const float *rays, uint32_t n, float time, float mint, float maxt,
                       uint32_t use_tree, int32_t *hit, float *t, uint32_t *visits);

/* Scene generators for the BASELINE configs.  Each fills caller arrays; call with
 * spheres == NULL to query the counts.  Returns RTW_OK or RTW_E_INVALID if capacity is too small. */
enum {
    RTW_SCENE_C1_THREE_SPHERES = 1, /* ground + lambert + metal (material_tests.rs:105-167 trimmed) */
    RTW_SCENE_C2_BOOK1_FINAL   = 2, /* Book-1 final random spheres, ~485                          */
    RTW_SCENE_C4_DIELECTRIC    = 4, /* 9x9 hollow-glass grid + fuzzy metal                         */
    RTW_SCENE_C5_MOTION_CHECKER= 5, /* C2 with moving lambert spheres + 4x2 image-textured ground  */
    RTW_SCENE_METAL_TEST       = 6, /* 4-sphere metal_test (material_tests.rs:105-167)             */
    RTW_SCENE_QUAD_TEST        = 7, /* the five quads of quad_test (objects/quad.rs:152-299)       */
    RTW_SCENE_PRESENTATION     = 8, /* presentation_image (main.rs:89-419): sphere + 6 quads (one a light) +
                                       a rotated smoke box + a rotated glass pane, black background  */
    RTW_SCENE_FIRST_FRAME      = 9  /* main()'s seven spheres (main.rs:427-496), the scene of Rust/First frame.png */
};
int rtw_scene_generate(uint32_t which, uint64_t scene_seed,
                       RtwSphere *spheres, uint32_t sphere_cap, uint32_t *n_spheres,
                       RtwTexture *textures, uint32_t texture_cap, uint32_t *n_textures,
                       float *texels, uint32_t texel_cap, uint32_t *n_texels);
/* Same for scenes with quads / instances (7, 8; the sphere-only ids work too).  Any output array may be NULL
 * when only the counts are wanted: counts[0..5) = spheres, quads, instances, inst_spheres, inst_quads
 * (these scenes carry no image textures). */
int rtw_scene_generate_geom(uint32_t which, uint64_t scene_seed, RtwSphere *spheres, RtwQuad *quads,
                            RtwInstance *instances, RtwSphere *inst_spheres, RtwQuad *inst_quads,
                            const uint32_t caps[5], uint32_t counts[5], float background[3]);
/* The camera + params each config is quoted with (width/height/samples/depth/lens/vfov/shutter). */
int rtw_scene_default_view(uint32_t which, RtwCamera *cam, RtwParams *params);

#ifdef __cplusplus
}
#endif
#endif /* RTW_H */
