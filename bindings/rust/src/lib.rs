//! Binding of `include/rtw.h` for the reference crate.  SOURCE ONLY (no Rust toolchain in the build
//! image).  Mirrors `Viewport::render` (Rust/src/viewport.rs:430) with the integrator chosen by enum:
//! a host closure cannot run on the GPU.
use std::os::raw::c_void;

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct RtwCamera { pub origin: [f32; 3], pub u: [f32; 3], pub v: [f32; 3], pub pixel00: [f32; 3],
    pub delta_u: [f32; 3], pub delta_v: [f32; 3], pub lens_radius: f32, pub time0: f32, pub shutter: f32 }

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct RtwSphere { pub center: [f32; 3], pub radius: f32, pub velocity: [f32; 3], pub col_mod: [f32; 3],
    pub tex_color: [f32; 3], pub metallicness: f32, pub opacity: f32, pub ir: f32, pub emitted: [f32; 3], pub tex: i32 }

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct RtwTexture { pub row: u32, pub col: u32, pub texel_offset: u32, pub emit_tex: u32 }   // emit_tex: 1 + index of Rust2's emission image, 0 = none

/// `Quad` (objects/quad.rs:8-20) + its Material; normal / d / w of Quad::new are recomputed by the library.
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct RtwQuad { pub origin: [f32; 3], pub u: [f32; 3], pub v: [f32; 3], pub velocity: [f32; 3], pub tex_color: [f32; 3],
    pub metallicness: f32, pub opacity: f32, pub ir: f32, pub emitted: [f32; 3], pub tex: i32 }

/// Rust2 `Triangle` (Rust2/src/objects/triangle.rs:12-50) + its Material; normal / d / w (Triangle::new) are written by
/// `Triangle::new` and recomputed by the library wherever it reads triangles.
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct RtwTriangle { pub origin: [f32; 3], pub u: [f32; 3], pub v: [f32; 3], pub normal: [f32; 3], pub d: f32, pub w: [f32; 3],
    pub tex_color: [f32; 3], pub metallicness: f32, pub opacity: f32, pub ir: f32, pub emitted: [f32; 3], pub tex: i32 }

/// One placement of the context's triangle mesh (rtw.h "mesh placements"): Rust2's `Instance` of triangles; quat = (w, x, y, z).
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct RtwMeshInstance { pub position: [f32; 3], pub quat: [f32; 4] }
pub const RTW_MAX_MESH_INSTANCES: u32 = 65536;
/// (t or +inf, placement or -1, triangle or -1, normal or 0) per ray
pub type MeshHits = (Vec<f32>, Vec<i32>, Vec<i32>, Vec<[f32; 3]>);

/// `Instance` (objects/instance.rs:27-38): member ranges into the scene's instance pools; medium 1 = const_density.
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct RtwInstance { pub first_sphere: u32, pub n_spheres: u32, pub first_quad: u32, pub n_quads: u32,
    pub translation: [f32; 3], pub rotation: [f32; 3], pub density: f32, pub medium: u32 }

#[repr(C)]
pub struct RtwScene { pub spheres: *const RtwSphere, pub textures: *const RtwTexture, pub texels: *const f32,
    pub n_spheres: u32, pub n_textures: u32, pub n_texels: u32, pub background: [f32; 3],
    pub quads: *const RtwQuad, pub instances: *const RtwInstance, pub inst_spheres: *const RtwSphere, pub inst_quads: *const RtwQuad,
    pub n_quads: u32, pub n_instances: u32, pub n_inst_spheres: u32, pub n_inst_quads: u32 }

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct RtwParams { pub width: u32, pub height: u32, pub samples: u32, pub depth: u32, pub gamma: f32,
    pub mint: f32, pub maxt: f32, pub integrator: u32, pub sampler: u32, pub accel: u32, pub flags: u32,
    pub seed: u64, pub row_block: u32, pub part_index: u32, pub part_count: u32, pub reserved: u32 }

#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtwStats { pub camera_rays: u64, pub segments: u64, pub sphere_tests: u64, pub node_tests: u64,
    pub nan_pixels: u32, pub rows: u32, pub kernel_ms: f32, pub total_ms: f32,
    pub phase_steps: [u64; 6], pub phase_lanes: [u64; 6], pub quad_tests: u64,
    pub enqueue_ms: f32, pub start_ms: f32 }      // ABI v4: the call's timeline (rtw.h)

/// `PerlinNoise` (texture.rs:61-68) without the never-read ranfloat; RtwPerlin::new(seed) == rtw_perlin_new (identity permutations).
#[repr(C)] #[derive(Clone, Copy)]
pub struct RtwPerlin { pub ranvec: [[f32; 3]; 256], pub perm_x: [u8; 256], pub perm_y: [u8; 256], pub perm_z: [u8; 256] }
/// Per texture: `ImageTexture.noise` (index into the tables, -1 = None) and `noise_scale` (texture.rs:21-27).
#[repr(C)] #[derive(Clone, Copy)]
pub struct RtwTextureNoise { pub perlin: i32, pub scale: f32 }

/// Arguments of the bilateral post-process (Rust2/src/postprocessing.rs:12-131): Proximity{size, type}, the input's format
/// (0 = [h][w][3] u8, 1 = the renderer's f32 frame, quantised first as Vec3::to_rgb_u8), the range term (0 = computed as the reference).
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct RtwBilateral { pub size: u32, pub proximity: u32, pub in_format: u32, pub avg_gradient: f32 }
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtwFilterStats { pub avg_gradient: f32, pub spatial: f32, pub gradient_ms: f32, pub table_ms: f32, pub filter_ms: f32,
    pub total_ms: f32, pub taps: u64 }
/// Arguments of the guided filter (include/rtw.h): the bilateral ones, the two sigmas (0 = term off) and same_object (1 = a tap on
/// another object id weighs 0).
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct RtwGuidedFilter { pub base: RtwBilateral, pub sigma_depth: f32, pub sigma_normal: f32, pub same_object: u32 }
/// Arguments of the a-trous filter (include/rtw.h): levels (1..8, level i steps by 2^i pixels), the three sigmas (0 = term off; level i uses
/// sigma_color * 2^-i), same_object, and the floor below which an albedo channel is not demodulated.
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct RtwAtrous { pub levels: u32, pub sigma_color: f32, pub sigma_depth: f32, pub sigma_normal: f32, pub same_object: u32, pub albedo_floor: f32 }
pub const RTW_ATROUS_MAX_LEVELS: u32 = 8;
/// Arguments of the variance estimate (include/rtw.h): the history length below which a pixel takes the spatial estimate (1 = never), its
/// window's radius (1..3), the two sigmas (0 = term off) and same_object.
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct RtwVarianceEstimate { pub min_history: u32, pub radius: u32, pub sigma_depth: f32, pub sigma_normal: f32, pub same_object: u32 }
pub const RTW_VARIANCE_MAX_RADIUS: u32 = 3;
/// What the variance-steered a-trous filter takes beside `RtwAtrous` (include/rtw.h): sigma_luminance (0 = term off), epsilon (> 0) and
/// prefilter (1 = the centre's variance is its 3 x 3 Gaussian mean).
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct RtwSvgf { pub sigma_luminance: f32, pub epsilon: f32, pub prefilter: u32 }
/// Arguments of the temporal accumulation (include/rtw.h): the two blend floors, the history cap, the depth and normal tests (0 = term
/// off), same_object and the RTW_RAYS_PIXEL offset of both frames' guides.
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct RtwTemporal { pub alpha: f32, pub alpha_moments: f32, pub max_history: u32, pub depth_tol: f32, pub normal_cos: f32,
    pub same_object: u32, pub offset: [f32; 2] }
/// One top-level object's rigid motion for the temporal accumulation with moving objects (include/rtw.h), 128 bytes: world points go
/// current -> previous by a (x - from) + to, the normals surface_map writes by nrm; moving 0: the rest of the row is not read.
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct RtwMotionRow { pub a: [f32; 9], pub from: [f32; 3], pub to: [f32; 3], pub nrm: [f32; 9], pub moving: u32, pub pad: [u32; 7] }
/// The buffers of one temporal accumulation (include/rtw.h "temporal accumulation"), each host memory or, for a context's call, device
/// memory of its GPU: the frame and its guides, the previous call's results and guides (all null on a first frame), the outputs
/// (out_variance and out_prev_xy may be null).  A guide whose term is off may be null.
#[repr(C)] #[derive(Clone, Copy)]
pub struct TemporalBuffers { pub cur: *const f32, pub depth: *const f32, pub normal: *const f32, pub idx: *const i32,
    pub prev_color: *const f32, pub prev_moments: *const f32, pub prev_len: *const f32, pub prev_depth: *const f32, pub prev_normal: *const f32,
    pub prev_idx: *const i32, pub out_color: *mut f32, pub out_moments: *mut f32, pub out_len: *mut f32, pub out_variance: *mut f32,
    pub out_prev_xy: *mut f32 }
/// `RTW_OPT_ATROUS_LAYOUT` (rtw.h): where a level of the a-trous filter reads its taps (0 the measured choice, 1 LDS tile, 2 global memory).
pub const RTW_OPT_ATROUS_LAYOUT: u32 = 14;
/// `RTW_OPT_HISTOGRAM_COUNT` (rtw.h): how the luminance histogram keeps its LDS counts (0 the measured choice, 1 plain, 2 per wave, 3 ballot).
pub const RTW_OPT_HISTOGRAM_COUNT: u32 = 15;
/// The ray rules of `rtw_ctx_surface_map` (rtw.h).
pub const RTW_RAYS_DEPTH_MAP: u32 = 0;
pub const RTW_RAYS_PIXEL: u32 = 1;
/// Rust2 `ProximityType` (postprocessing.rs:12-15).
#[repr(u32)] #[derive(Clone, Copy)]
pub enum ProximityKind { Square = 0, Edges = 1 }
/// Rust2 `Proximity::new(size, type)` (postprocessing.rs:23-29); size <= 64.
#[derive(Clone, Copy)]
pub struct Proximity { pub size: u32, pub kind: ProximityKind }
impl Proximity { pub fn new(size: u32, kind: ProximityKind) -> Self { Self { size, kind } } }

#[repr(C)] pub struct RtwCtx { _private: [u8; 0] }
#[repr(C)] pub struct RtwMgpu { _private: [u8; 0] }

#[repr(u32)] #[derive(Clone, Copy)]
pub enum Integrator { Gradient = 0, BgColor = 1, Normal = 2, Flag = 3, Rust2 = 4, LightCast = 5, LightBiased = 6 }   // ray_color.rs:12-92; Rust2/src/viewport/ray_color.rs:12-37, :55-164
/// A light of Rust2's light-biased integrators: a top-level sphere (kind 0) or quad (kind 1) of the scene (rtw.h RtwLight).
#[repr(C)] #[derive(Clone, Copy)]
pub struct RtwLight { pub kind: u32, pub index: u32 }
pub const RTW_MAX_LIGHTS: usize = 16;
/// RtwParams.flags bit (rtw.h): under the Rust2 integrators an object with opacity < 0 is `MixedMaterial::new(ir)`
/// (Rust2/src/objects/material.rs:235-297), i.e. material triple (0, -1, exp).
pub const RTW_FLAG_MIXED_MATERIAL: u32 = 32;
#[repr(u32)] #[derive(Clone, Copy)]
pub enum Sampler { Row = 0, Stratified = 1, Centres = 2, NoRand = 3 }      // viewport.rs:270-305, 430-516

/// `RTW_OPT_MESH_LIST_MAX` (rtw.h): the option key of the placement count up to which placements are met in list order.
pub const RTW_OPT_MESH_LIST_MAX: u32 = 12;
/// `RTW_OPT_MESH_CLIMB` (rtw.h): how `move_mesh_instances` climbs the top-level tree (0 by node count, 1 per height, 2 one workgroup).
pub const RTW_OPT_MESH_CLIMB: u32 = 13;
/// A node of the top-level tree over mesh placements (rtw.h `RtwTriNode`): leaf = (first << 3) | count, 0 for an inner node.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct RtwTriNode { pub lo: [f32; 3], pub skip: u32, pub hi: [f32; 3], pub leaf: u32 }

/// One wrong result of a device sweep (rtw.h `RtwSweepResult.records`): bit patterns of the arguments (b = 0 for sqrt) and of what came back.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct RtwSweepRecord { pub a: u32, pub b: u32, pub got: u32, pub reserved: u32 }
/// What `rtw_ctx_device_sweep` reports (rtw.h "device math, for tests").
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct RtwSweepResult {
    pub tested: u64, pub wrong: u64, pub n_records: u32, pub reserved: u32, pub records: [RtwSweepRecord; 16], pub kernel_ms: f32, pub reserved2: u32,
}
/// `rtw_ctx_device_math`'s functions: (fn, columns read, columns written)
pub const RTW_MATH_SQRT_PLAIN: (u32, u32, u32) = (0, 1, 1);
pub const RTW_MATH_SQRT_IEEE: (u32, u32, u32) = (1, 1, 1);
pub const RTW_MATH_DIV: (u32, u32, u32) = (2, 2, 1);
pub const RTW_MATH_UNIT: (u32, u32, u32) = (3, 3, 3);
pub const RTW_MATH_UNIT_BALL: (u32, u32, u32) = (4, 4, 3);
pub const RTW_MATH_SPHERE_ROOT: (u32, u32, u32) = (5, 4, 1);
pub const RTW_MATH_ATAN2: (u32, u32, u32) = (6, 2, 1);
pub const RTW_MATH_ACOS: (u32, u32, u32) = (7, 1, 1);
pub const RTW_MATH_SPHERE_UV: (u32, u32, u32) = (8, 3, 2);
pub const RTW_MATH_LN: (u32, u32, u32) = (9, 1, 1);
pub const RTW_MATH_POW: (u32, u32, u32) = (10, 2, 1);
pub const RTW_MATH_SINCOS: (u32, u32, u32) = (11, 1, 2);
pub const RTW_MATH_EXP: (u32, u32, u32) = (12, 1, 1);
pub const RTW_SWEEP_SQRT: u32 = 0;
pub const RTW_SWEEP_DIV_RANDOM: u32 = 1;
pub const RTW_SWEEP_DIV_MIDPOINT: u32 = 2;

extern "C" {
    fn rtw_ctx_device_math(ctx: *mut RtwCtx, func: u32, input: *const f32, n_cols: u32, n: u32, out: *mut f32, out_cols: u32) -> i32;
    fn rtw_ctx_device_sweep(ctx: *mut RtwCtx, which: u32, first: u64, count: u64, seed: u32, result: *mut RtwSweepResult) -> i32;
    fn rtw_rounding_check(which: u32, a: *const u32, b: *const u32, got: *const u32, n: usize, ok: *mut u8) -> i32;
    fn rtw_sweep_operands(which: u32, first: u64, n: usize, seed: u32, out: *mut u32) -> i32;
    fn rtw_ctx_create(device: i32, out: *mut *mut RtwCtx) -> i32;
    fn rtw_ctx_destroy(ctx: *mut RtwCtx);
    fn rtw_ctx_set_scene(ctx: *mut RtwCtx, scene: *const RtwScene, t_begin: f32, t_end: f32) -> i32;
    fn rtw_ctx_render(ctx: *mut RtwCtx, cam: *const RtwCamera, p: *const RtwParams, out_rgb: *mut c_void, st: *mut RtwStats) -> i32;
    fn rtw_ctx_render_multi(ctx: *mut RtwCtx, cam: *const RtwCamera, p: *const RtwParams, fps: f32, start_frame: u32, n_frames: u32,
                            out_rgb: *mut c_void, st: *mut RtwStats) -> i32;
    fn rtw_strerror(status: i32) -> *const std::os::raw::c_char;
    fn rtw_part_rows(height: u32, row_block: u32, part_index: u32, part_count: u32) -> u32;
    fn rtw_ctx_set_option(ctx: *mut RtwCtx, key: u32, value: f64) -> i32;
    fn rtw_ctx_last_node_format(ctx: *mut RtwCtx) -> i32;
    fn rtw_mgpu_create(devices: *const i32, n: u32, out: *mut *mut RtwMgpu) -> i32;
    fn rtw_mgpu_destroy(m: *mut RtwMgpu);
    fn rtw_mgpu_set_scene(m: *mut RtwMgpu, scene: *const RtwScene, t_begin: f32, t_end: f32) -> i32;
    fn rtw_perlin_new(seed: u64, out: *mut RtwPerlin) -> i32;
    fn rtw_perlin_eval(t: *const RtwPerlin, points: *const f32, n: u32, turb_depth: u32, out: *mut f32) -> i32;
    fn rtw_ctx_perlin_eval(ctx: *mut RtwCtx, t: *const RtwPerlin, points: *const f32, n: u32, turb_depth: u32, out: *mut f32) -> i32;
    fn rtw_ctx_set_texture_noise(ctx: *mut RtwCtx, tables: *const RtwPerlin, n_tables: u32,
                                 per_texture: *const RtwTextureNoise, n_textures: u32) -> i32;
    fn rtw_mgpu_set_texture_noise(m: *mut RtwMgpu, tables: *const RtwPerlin, n_tables: u32,
                                  per_texture: *const RtwTextureNoise, n_textures: u32) -> i32;
    fn rtw_bilateral_filter(img: *const c_void, w: u32, h: u32, p: *const RtwBilateral, out: *mut u8, st: *mut RtwFilterStats) -> i32;
    fn rtw_ctx_bilateral_filter(ctx: *mut RtwCtx, img: *const c_void, w: u32, h: u32, p: *const RtwBilateral, out: *mut u8,
                                st: *mut RtwFilterStats) -> i32;
    fn rtw_guided_filter(img: *const c_void, w: u32, h: u32, depth: *const f32, normal: *const f32, idx: *const i32,
                             p: *const RtwGuidedFilter, out: *mut u8, st: *mut RtwFilterStats) -> i32;
    fn rtw_ctx_guided_filter(ctx: *mut RtwCtx, img: *const c_void, w: u32, h: u32, depth: *const f32, normal: *const f32,
                                 idx: *const i32, p: *const RtwGuidedFilter, out: *mut u8, st: *mut RtwFilterStats) -> i32;
    fn rtw_atrous_filter(img: *const f32, w: u32, h: u32, depth: *const f32, normal: *const f32, idx: *const i32, albedo: *const f32,
                         emitted: *const f32, p: *const RtwAtrous, out: *mut f32, st: *mut RtwFilterStats) -> i32;
    fn rtw_ctx_atrous_filter(ctx: *mut RtwCtx, img: *const f32, w: u32, h: u32, depth: *const f32, normal: *const f32, idx: *const i32,
                             albedo: *const f32, emitted: *const f32, p: *const RtwAtrous, out: *mut f32, st: *mut RtwFilterStats) -> i32;
    fn rtw_variance_estimate(moments: *const f32, len: *const f32, w: u32, h: u32, depth: *const f32, normal: *const f32, idx: *const i32,
                             p: *const RtwVarianceEstimate, out: *mut f32, st: *mut RtwFilterStats) -> i32;
    fn rtw_ctx_variance_estimate(ctx: *mut RtwCtx, moments: *const f32, len: *const f32, w: u32, h: u32, depth: *const f32, normal: *const f32,
                                 idx: *const i32, p: *const RtwVarianceEstimate, out: *mut f32, st: *mut RtwFilterStats) -> i32;
    fn rtw_svgf_filter(img: *const f32, variance: *const f32, w: u32, h: u32, depth: *const f32, normal: *const f32, idx: *const i32,
                       albedo: *const f32, emitted: *const f32, p: *const RtwAtrous, vp: *const RtwSvgf, out: *mut f32, out_variance: *mut f32,
                       st: *mut RtwFilterStats) -> i32;
    fn rtw_ctx_svgf_filter(ctx: *mut RtwCtx, img: *const f32, variance: *const f32, w: u32, h: u32, depth: *const f32, normal: *const f32,
                           idx: *const i32, albedo: *const f32, emitted: *const f32, p: *const RtwAtrous, vp: *const RtwSvgf, out: *mut f32,
                           out_variance: *mut f32, st: *mut RtwFilterStats) -> i32;
    fn rtw_temporal_accumulate_motion(cur: *const f32, w: u32, h: u32, cam: *const RtwCamera, depth: *const f32, normal: *const f32,
                                      idx: *const i32, prev_cam: *const RtwCamera, prev_color: *const f32, prev_moments: *const f32,
                                      prev_len: *const f32, prev_depth: *const f32, prev_normal: *const f32, prev_idx: *const i32,
                                      p: *const RtwTemporal, rows: *const RtwMotionRow, n_rows: u32, first: u32, out_color: *mut f32,
                                      out_moments: *mut f32, out_len: *mut f32, out_variance: *mut f32, out_prev_xy: *mut f32,
                                      st: *mut RtwFilterStats) -> i32;
    fn rtw_ctx_temporal_accumulate_motion(ctx: *mut RtwCtx, cur: *const f32, w: u32, h: u32, cam: *const RtwCamera, depth: *const f32,
                                          normal: *const f32, idx: *const i32, prev_cam: *const RtwCamera, prev_color: *const f32,
                                          prev_moments: *const f32, prev_len: *const f32, prev_depth: *const f32, prev_normal: *const f32,
                                          prev_idx: *const i32, p: *const RtwTemporal, rows: *const RtwMotionRow, n_rows: u32, first: u32,
                                          out_color: *mut f32, out_moments: *mut f32, out_len: *mut f32, out_variance: *mut f32,
                                          out_prev_xy: *mut f32, st: *mut RtwFilterStats) -> i32;
    fn rtw_mesh_instance_motion(prev_poses: *const f32, cur_poses: *const f32, n: u32, rows_out: *mut RtwMotionRow, n_invalid: *mut u32) -> i32;
    fn rtw_ctx_mesh_instance_motion(ctx: *mut RtwCtx, prev_poses: *const f32, cur_poses: *const f32, n: u32, rows_out: *mut RtwMotionRow,
                                    n_invalid: *mut u32) -> i32;
    // per-pixel motion (rtw.h "temporal accumulation with per-pixel motion"): declared for callers of the raw ABI; no safe wrapper yet
    #[allow(dead_code)]
    fn rtw_deform_motion(tri: *const i32, bary: *const f32, n: u32, prev_ouv: *const f32, n_tris: u32, idx: *const i32, prev_poses: *const f32,
                         n_mesh: u32, first: u32, prev_point_out: *mut f32, carried_normal_out: *mut f32) -> i32;
    #[allow(dead_code)]
    fn rtw_ctx_deform_motion(ctx: *mut RtwCtx, tri: *const i32, bary: *const f32, n: u32, prev_ouv: *const f32, n_tris: u32, idx: *const i32,
                             prev_poses: *const f32, n_mesh: u32, first: u32, prev_point_out: *mut f32, carried_normal_out: *mut f32) -> i32;
    #[allow(dead_code)]
    fn rtw_ctx_temporal_accumulate_points(ctx: *mut RtwCtx, cur: *const f32, w: u32, h: u32, cam: *const RtwCamera, depth: *const f32,
                                          normal: *const f32, idx: *const i32, prev_cam: *const RtwCamera, prev_color: *const f32,
                                          prev_moments: *const f32, prev_len: *const f32, prev_depth: *const f32, prev_normal: *const f32,
                                          prev_idx: *const i32, p: *const RtwTemporal, rows: *const RtwMotionRow, n_rows: u32, first: u32,
                                          prev_point: *const f32, carried_normal: *const f32, out_color: *mut f32, out_moments: *mut f32,
                                          out_len: *mut f32, out_variance: *mut f32, out_prev_xy: *mut f32, st: *mut RtwFilterStats) -> i32;
    #[allow(dead_code)]
    fn rtw_ctx_surface_map_tri(ctx: *mut RtwCtx, cam: *const RtwCamera, width: u32, height: u32, ray_rule: u32, offset: *const f32, time: f32,
                               mint: f32, maxt: f32, accel: u32, integrator: u32, depth_out: *mut f32, idx_out: *mut i32, normal_out: *mut f32,
                               albedo_out: *mut f32, emitted_out: *mut f32, material_out: *mut f32, tri_out: *mut i32, bary_out: *mut f32,
                               stats: *mut RtwStats) -> i32;
    fn rtw_triangle_new(origin: *const f32, u: *const f32, v: *const f32, mat3: *const f32, emitted: *const f32,
                        color: *const f32, tex: i32, out: *mut RtwTriangle) -> i32;
    fn rtw_ctx_set_triangles(ctx: *mut RtwCtx, tris: *const RtwTriangle, n: u32) -> i32;
    fn rtw_ctx_set_lights(ctx: *mut RtwCtx, lights: *const RtwLight, n: u32, biased_weight: f32) -> i32;
    fn rtw_mgpu_set_lights(m: *mut RtwMgpu, lights: *const RtwLight, n: u32, biased_weight: f32) -> i32;
    fn rtw_mgpu_set_triangles(m: *mut RtwMgpu, tris: *const RtwTriangle, n: u32) -> i32;
    fn rtw_ctx_set_instance_rotations(ctx: *mut RtwCtx, quat: *const [f32; 4], n: u32) -> i32;
    fn rtw_mgpu_set_instance_rotations(m: *mut RtwMgpu, quat: *const [f32; 4], n: u32) -> i32;
    fn rtw_ctx_set_mesh_instances(ctx: *mut RtwCtx, p: *const RtwMeshInstance, n: u32) -> i32;
    fn rtw_mgpu_set_mesh_instances(m: *mut RtwMgpu, p: *const RtwMeshInstance, n: u32) -> i32;
    fn rtw_mesh_instances_validate(tris: *const RtwTriangle, n_tris: u32, p: *const RtwMeshInstance, n: u32) -> i32;
    fn rtw_mesh_instance_hits(tris: *const RtwTriangle, n_tris: u32, p: *const RtwMeshInstance, n: u32, rays: *const f32, n_rays: u32,
                              mint: f32, maxt: f32, t_out: *mut f32, placement_out: *mut i32, tri_out: *mut i32, normal_out: *mut f32) -> i32;
    fn rtw_ctx_mesh_instance_hits(ctx: *mut RtwCtx, rays: *const f32, n_rays: u32, mint: f32, maxt: f32, accel: u32, t_out: *mut f32,
                                  placement_out: *mut i32, tri_out: *mut i32, normal_out: *mut f32, stats: *mut RtwStats) -> i32;
    fn rtw_mesh_list_max_default() -> u32;
    fn rtw_mesh_top_dump(tris: *const RtwTriangle, n_tris: u32, p: *const RtwMeshInstance, n: u32, nodes_out: *mut RtwTriNode, node_cap: u32,
                         n_nodes: *mut u32, order_out: *mut u32, depth: *mut u32, list_walk: *mut u32) -> i32;
    fn rtw_ctx_refit_triangles(ctx: *mut RtwCtx, ouv: *const f32, n: u32, list_walk_out: *mut u32) -> i32;
    fn rtw_ctx_triangle_bvh_dump(ctx: *mut RtwCtx, nodes_out: *mut RtwTriNode, node_cap: u32, n_nodes: *mut u32) -> i32;
    fn rtw_triangle_bvh_dump(tris: *const RtwTriangle, n: u32, nodes_out: *mut RtwTriNode, node_cap: u32, n_nodes: *mut u32, order_out: *mut u32,
                             depth: *mut u32, list_walk: *mut u32) -> i32;
    fn rtw_triangle_bvh_refit(tris: *const RtwTriangle, n: u32, ouv: *const f32, nodes_out: *mut RtwTriNode, node_cap: u32, n_nodes: *mut u32,
                              list_walk: *mut u32) -> i32;
    fn rtw_ctx_move_mesh_instances(ctx: *mut RtwCtx, poses: *const f32, n: u32, ouv: *const f32, n_tris: u32, list_walk_out: *mut u32) -> i32;
    fn rtw_ctx_mesh_top_dump(ctx: *mut RtwCtx, nodes_out: *mut RtwTriNode, node_cap: u32, n_nodes: *mut u32, rows_out: *mut f32) -> i32;
    fn rtw_mesh_top_refit(tris: *const RtwTriangle, n_tris: u32, p: *const RtwMeshInstance, n: u32, moved: *const f32, ouv: *const f32,
                          nodes_out: *mut RtwTriNode, node_cap: u32, n_nodes: *mut u32, rows_out: *mut f32, list_walk: *mut u32,
                          n_invalid: *mut u32) -> i32;
    fn rtw_mesh_instance_hits_tree(tris: *const RtwTriangle, n_tris: u32, p: *const RtwMeshInstance, n: u32, rays: *const f32, n_rays: u32,
                                   mint: f32, maxt: f32, t_out: *mut f32, placement_out: *mut i32, tri_out: *mut i32, normal_out: *mut f32,
                                   stats: *mut RtwStats) -> i32;
    fn rtw_quat_rotate(q: *const f32, v: *const f32, out: *mut f32) -> i32;
    fn rtw_quat_mul(a: *const f32, b: *const f32, out: *mut f32) -> i32;
    fn rtw_quat_from_axis(angle: f32, axis: *const f32, out: *mut f32) -> i32;
    fn rtw_quat_from_euler(euler: *const f32, out: *mut f32) -> i32;
    fn rtw_triangle_hits(tris: *const RtwTriangle, n: u32, rays: *const f32, n_rays: u32, mint: f32, maxt: f32,
                         t_out: *mut f32, idx_out: *mut i32) -> i32;
    fn rtw_ctx_triangle_hits(ctx: *mut RtwCtx, rays: *const f32, n_rays: u32, mint: f32, maxt: f32, accel: u32,
                             t_out: *mut f32, idx_out: *mut i32, stats: *mut RtwStats) -> i32;
    fn rtw_camera2_new(aspect: f32, origin: *const f32, vup: *const f32, dir: *const f32, vfov: f32, lens_radius: f32, cam: *mut RtwCamera) -> i32;
    fn rtw_depth_rays(cam: *const RtwCamera, width: u32, height: u32, rays_out: *mut f32) -> i32;
    fn rtw_ctx_scene_hits(ctx: *mut RtwCtx, rays: *const f32, n_rays: u32, time: f32, mint: f32, maxt: f32, accel: u32,
                          t_out: *mut f32, idx_out: *mut i32, normal_out: *mut f32, stats: *mut RtwStats) -> i32;
    fn rtw_ctx_scene_surface(ctx: *mut RtwCtx, rays: *const f32, n_rays: u32, time: f32, mint: f32, maxt: f32, accel: u32, integrator: u32,
                             t_out: *mut f32, idx_out: *mut i32, normal_out: *mut f32, albedo_out: *mut f32, emitted_out: *mut f32,
                             material_out: *mut f32, stats: *mut RtwStats) -> i32;
    fn rtw_pixel_rays(cam: *const RtwCamera, width: u32, height: u32, offset: *const f32, rays_out: *mut f32) -> i32;
    fn rtw_ctx_surface_map(ctx: *mut RtwCtx, cam: *const RtwCamera, width: u32, height: u32, ray_rule: u32, offset: *const f32, time: f32,
                           mint: f32, maxt: f32, accel: u32, integrator: u32, depth_out: *mut f32, idx_out: *mut i32, normal_out: *mut f32,
                           albedo_out: *mut f32, emitted_out: *mut f32, material_out: *mut f32, stats: *mut RtwStats) -> i32;
    fn rtw_ctx_scene_occluded(ctx: *mut RtwCtx, rays: *const f32, n_rays: u32, time: f32, mint: f32, maxt: f32, accel: u32,
                              occluded_out: *mut u8, stats: *mut RtwStats) -> i32;
    fn rtw_ao_rays(points: *const f32, normals: *const f32, n: u32, samples: u32, seed: u32, rays_out: *mut f32) -> i32;
    fn rtw_ctx_ambient_occlusion(ctx: *mut RtwCtx, points: *const f32, normals: *const f32, n: u32, samples: u32, seed: u32, time: f32,
                                 mint: f32, maxt: f32, accel: u32, ao_out: *mut f32, stats: *mut RtwStats) -> i32;
    fn rtw_ctx_ao_map(ctx: *mut RtwCtx, cam: *const RtwCamera, width: u32, height: u32, time: f32, mint: f32, maxt: f32, samples: u32,
                      seed: u32, ao_mint: f32, ao_maxt: f32, accel: u32, ao_out: *mut f32, depth_out: *mut f32, idx_out: *mut i32,
                      normal_out: *mut f32, stats: *mut RtwStats) -> i32;
    fn rtw_ctx_depth_map(ctx: *mut RtwCtx, cam: *const RtwCamera, width: u32, height: u32, time: f32, mint: f32, maxt: f32, accel: u32,
                         depth_out: *mut f32, idx_out: *mut i32, normal_out: *mut f32, stats: *mut RtwStats) -> i32;
    fn rtw_mgpu_render(m: *mut RtwMgpu, cam: *const RtwCamera, p: *const RtwParams, out_rgb: *mut c_void,
                       per_device: *mut RtwStats, total: *mut RtwStats) -> i32;
}

#[derive(Debug)]
pub struct RtwError(pub i32);
impl std::fmt::Display for RtwError {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        let s = unsafe { std::ffi::CStr::from_ptr(rtw_strerror(self.0)) };
        write!(f, "rtw: {}", s.to_string_lossy())
    }
}
fn check(rc: i32) -> Result<(), RtwError> { if rc == 0 { Ok(()) } else { Err(RtwError(rc)) } }

/// One GPU.  `Renderer::new(0)?.set_scene(..)?.render(..)` replaces `viewport.render(&ray_color, &scene)`.
pub struct Renderer { ctx: *mut RtwCtx }
impl Renderer {
    pub fn new(device: i32) -> Result<Self, RtwError> {
        let mut ctx = std::ptr::null_mut();
        check(unsafe { rtw_ctx_create(device, &mut ctx) })?;
        Ok(Self { ctx })
    }
    /// == Scene::new_sphere(spheres) (viewport.rs:90-105); `texels` is the concatenation of every
    /// ImageTexture.img (texture.rs:21-27), `textures[i]` = {row, col, offset}.
    pub fn set_scene(&mut self, spheres: &[RtwSphere], textures: &[RtwTexture], texels: &[[f32; 3]],
                     background: [f32; 3], t_begin: f32, t_end: f32) -> Result<(), RtwError> {
        let sc = RtwScene { spheres: spheres.as_ptr(), textures: textures.as_ptr(), texels: texels.as_ptr() as *const f32,
            n_spheres: spheres.len() as u32, n_textures: textures.len() as u32, n_texels: texels.len() as u32, background,
            quads: std::ptr::null(), instances: std::ptr::null(), inst_spheres: std::ptr::null(), inst_quads: std::ptr::null(),
            n_quads: 0, n_instances: 0, n_inst_spheres: 0, n_inst_quads: 0 };
        check(unsafe { rtw_ctx_set_scene(self.ctx, &sc, t_begin, t_end) })
    }
    /// == Scene::new(spheres, quads, instances) (viewport.rs:122-135).  `inst_spheres` / `inst_quads` are the member pools
    /// the instances' ranges index (Instance{spheres, quads} flattened in instance order).
    pub fn set_scene_full(&mut self, spheres: &[RtwSphere], quads: &[RtwQuad], instances: &[RtwInstance],
                          inst_spheres: &[RtwSphere], inst_quads: &[RtwQuad], textures: &[RtwTexture], texels: &[[f32; 3]],
                          background: [f32; 3], t_begin: f32, t_end: f32) -> Result<(), RtwError> {
        let sc = RtwScene { spheres: spheres.as_ptr(), textures: textures.as_ptr(), texels: texels.as_ptr() as *const f32,
            n_spheres: spheres.len() as u32, n_textures: textures.len() as u32, n_texels: texels.len() as u32, background,
            quads: quads.as_ptr(), instances: instances.as_ptr(), inst_spheres: inst_spheres.as_ptr(), inst_quads: inst_quads.as_ptr(),
            n_quads: quads.len() as u32, n_instances: instances.len() as u32,
            n_inst_spheres: inst_spheres.len() as u32, n_inst_quads: inst_quads.len() as u32 };
        check(unsafe { rtw_ctx_set_scene(self.ctx, &sc, t_begin, t_end) })
    }
    /// ImageTexture{noise, noise_scale} of the scene just set (per_texture[i] for its texture i; an empty slice clears it).
    /// set_scene clears it; RTW_INTEGRATOR_RUST2 is refused while a used texture has noise.
    pub fn set_texture_noise(&mut self, tables: &[RtwPerlin], per_texture: &[RtwTextureNoise]) -> Result<(), RtwError> {
        let (t, pt) = if per_texture.is_empty() { (std::ptr::null(), std::ptr::null()) } else { (tables.as_ptr(), per_texture.as_ptr()) };
        check(unsafe { rtw_ctx_set_texture_noise(self.ctx, t, tables.len() as u32, pt, per_texture.len() as u32) })
    }
    /// Rust2 triangles of the scene just set (an empty slice clears them); set_scene clears them.  Builds their tree: RTW_ACCEL_BVH
    /// renders use it, RTW_ACCEL_BRUTE renders walk the list -- the same image.  Refused (RTW_E_UNSUPPORTED) while texture noise is set.
    pub fn set_triangles(&mut self, tris: &[RtwTriangle]) -> Result<(), RtwError> {
        let p = if tris.is_empty() { std::ptr::null() } else { tris.as_ptr() };
        check(unsafe { rtw_ctx_set_triangles(self.ctx, p, tris.len() as u32) })
    }
    /// rtw_ctx_refit_triangles: move the context's triangles to `ouv` (origin, u, v per triangle, list order; host memory here, staged) and
    /// refit their tree on the GPU; topology, materials and order stay.  Ok(true): a triangle now breaks a condition of the tree and the
    /// context walks the list.  Refused (RTW_E_INVALID) for another count than the context's and while placements are set.
    pub fn refit_triangles(&mut self, ouv: &[[f32; 9]]) -> Result<bool, RtwError> {
        let mut walk = 0u32;
        check(unsafe { rtw_ctx_refit_triangles(self.ctx, ouv.as_ptr() as *const f32, ouv.len() as u32, &mut walk) })?;
        Ok(walk != 0)
    }
    /// rtw_ctx_move_mesh_instances: give the context's placements new poses (position xyz, quat wxyz each; None: they stay) and / or its mesh
    /// new triangles (`ouv` as refit_triangles takes it; None: the mesh stays) and refit both trees on the GPU; host memory here, staged.
    /// Ok(list_walk): bit 0 a triangle breaks a condition of the mesh's tree, bit 1 a placement lies beyond reach and the placements are met
    /// in list order.  An invalid pose leaves its placement where it was and the call answers RTW_E_INVALID.
    pub fn move_mesh_instances(&mut self, poses: Option<&[[f32; 7]]>, ouv: Option<&[[f32; 9]]>) -> Result<u32, RtwError> {
        let mut walk = 0u32;
        let (pp, pn) = poses.map_or((std::ptr::null(), 0), |p| (p.as_ptr() as *const f32, p.len() as u32));
        let (op, on) = ouv.map_or((std::ptr::null(), 0), |o| (o.as_ptr() as *const f32, o.len() as u32));
        check(unsafe { rtw_ctx_move_mesh_instances(self.ctx, pp, pn, op, on, &mut walk) })?;
        Ok(walk)
    }
    /// rtw_ctx_triangle_bvh_dump: the nodes of the context's triangle tree as the device holds them now.
    pub fn triangle_bvh_dump(&mut self) -> Result<Vec<RtwTriNode>, RtwError> {
        let mut n = 0u32;
        check(unsafe { rtw_ctx_triangle_bvh_dump(self.ctx, std::ptr::null_mut(), 0, &mut n) })?;
        let mut nodes = vec![RtwTriNode::default(); n as usize];
        check(unsafe { rtw_ctx_triangle_bvh_dump(self.ctx, nodes.as_mut_ptr(), n, std::ptr::null_mut()) })?;
        Ok(nodes)
    }
    /// The `lights` / `biased_weight` captures of Rust2's light_biased_ray_cast / light_biased_ray_color closures (an empty slice clears
    /// them; set_scene clears them): Integrator::LightCast / LightBiased then send one shadow ray per light from every surface hit.
    pub fn set_lights(&mut self, lights: &[RtwLight], biased_weight: f32) -> Result<(), RtwError> {
        let p = if lights.is_empty() { std::ptr::null() } else { lights.as_ptr() };
        check(unsafe { rtw_ctx_set_lights(self.ctx, p, lights.len() as u32, biased_weight) })
    }
    /// Rust2's `Instance.rotation`, one quaternion [w, x, y, z] per instance of the scene (`Instance::getr()`; an empty slice clears them;
    /// set_scene clears them): Integrator::Rust2 / LightCast / LightBiased and the scene queries then hit the instances as Rust2's
    /// `Instance::get_hit` does.
    pub fn set_instance_rotations(&mut self, quats: &[[f32; 4]]) -> Result<(), RtwError> {
        let p = if quats.is_empty() { std::ptr::null() } else { quats.as_ptr() };
        check(unsafe { rtw_ctx_set_instance_rotations(self.ctx, p, quats.len() as u32) })
    }
    /// rtw_ctx_set_mesh_instances: place the context's triangle mesh at every placement (empty: clear).  Renders under
    /// RTW_INTEGRATOR_RUST2 and the scene queries honour them; set_scene and set_triangles clear them.
    pub fn set_mesh_instances(&mut self, placements: &[RtwMeshInstance]) -> Result<(), RtwError> {
        let p = if placements.is_empty() { std::ptr::null() } else { placements.as_ptr() };
        check(unsafe { rtw_ctx_set_mesh_instances(self.ctx, p, placements.len() as u32) })
    }
    /// The closest placement of this context's mesh per ray on its GPU (rtw_ctx_mesh_instance_hits).
    pub fn mesh_instance_hits(&mut self, rays: &[[f32; 6]], mint: f32, maxt: f32, accel: u32) -> Result<MeshHits, RtwError> {
        let n = rays.len();
        let (mut t, mut p, mut i, mut nr) = (vec![0f32; n], vec![0i32; n], vec![0i32; n], vec![[0f32; 3]; n]);
        check(unsafe { rtw_ctx_mesh_instance_hits(self.ctx, rays.as_ptr() as *const f32, n as u32, mint, maxt, accel, t.as_mut_ptr(),
                                                  p.as_mut_ptr(), i.as_mut_ptr(), nr.as_mut_ptr() as *mut f32, std::ptr::null_mut()) })?;
        Ok((t, p, i, nr))
    }
    /// The closest of this context's triangles per ray ([origin, direction]) on its GPU: (t, index or -1) per ray.
    pub fn triangle_hits(&mut self, rays: &[[f32; 6]], mint: f32, maxt: f32, accel: u32) -> Result<(Vec<f32>, Vec<i32>), RtwError> {
        let (mut t, mut i) = (vec![0f32; rays.len()], vec![0i32; rays.len()]);
        check(unsafe { rtw_ctx_triangle_hits(self.ctx, rays.as_ptr() as *const f32, rays.len() as u32, mint, maxt, accel,
                                             t.as_mut_ptr(), i.as_mut_ptr(), std::ptr::null_mut()) })?;
        Ok((t, i))
    }
    /// The closest hit of each ray ([origin, direction], the direction not normalised) against the whole scene -- spheres, quads,
    /// instances, triangles; constant-density instances are skipped --: (t or +inf, top-level index or -1, outward normal or 0) per ray.
    pub fn scene_hits(&mut self, rays: &[[f32; 6]], time: f32, mint: f32, maxt: f32, accel: u32)
                      -> Result<(Vec<f32>, Vec<i32>, Vec<[f32; 3]>), RtwError> {
        let (mut t, mut i, mut n) = (vec![0f32; rays.len()], vec![0i32; rays.len()], vec![[0f32; 3]; rays.len()]);
        check(unsafe { rtw_ctx_scene_hits(self.ctx, rays.as_ptr() as *const f32, rays.len() as u32, time, mint, maxt, accel,
                                          t.as_mut_ptr(), i.as_mut_ptr(), n.as_mut_ptr() as *mut f32, std::ptr::null_mut()) })?;
        Ok((t, i, n))
    }
    /// Is anything of the whole scene in the way of each ray within [mint, maxt]?  The any-hit pass: `true` exactly where `scene_hits`
    /// reports an index >= 0, with the early exit a closest-hit query cannot take.
    pub fn scene_occluded(&mut self, rays: &[[f32; 6]], time: f32, mint: f32, maxt: f32, accel: u32) -> Result<Vec<bool>, RtwError> {
        let mut o = vec![0u8; rays.len()];
        check(unsafe { rtw_ctx_scene_occluded(self.ctx, rays.as_ptr() as *const f32, rays.len() as u32, time, mint, maxt, accel,
                                              o.as_mut_ptr(), std::ptr::null_mut()) })?;
        Ok(o.into_iter().map(|b| b != 0).collect())
    }
    /// Ambient occlusion of `points` with `normals`: the share of `samples` cosine-weighted rays about each normal that nothing stops
    /// within [mint, maxt], made and walked in one kernel.  `samples`: a power of two in 1 ..= 1024.
    pub fn ambient_occlusion(&mut self, points: &[[f32; 3]], normals: &[[f32; 3]], samples: u32, seed: u32, time: f32, mint: f32, maxt: f32,
                             accel: u32) -> Result<Vec<f32>, RtwError> {
        if points.len() != normals.len() { return Err(RtwError(-1)); }
        let mut ao = vec![0f32; points.len()];
        check(unsafe { rtw_ctx_ambient_occlusion(self.ctx, points.as_ptr() as *const f32, normals.as_ptr() as *const f32, points.len() as u32,
                                                 samples, seed, time, mint, maxt, accel, ao.as_mut_ptr(), std::ptr::null_mut()) })?;
        Ok(ao)
    }
    /// `depth_map` and then `ambient_occlusion` of its hit points over [ao_mint, ao_maxt], in two launches: row-major [height][width],
    /// 1.0 for a miss pixel.
    pub fn ao_map(&mut self, cam: &RtwCamera, width: u32, height: u32, time: f32, mint: f32, maxt: f32, samples: u32, seed: u32, ao_mint: f32,
                  ao_maxt: f32, accel: u32) -> Result<Vec<f32>, RtwError> {
        let mut ao = vec![0f32; width as usize * height as usize];
        check(unsafe { rtw_ctx_ao_map(self.ctx, cam, width, height, time, mint, maxt, samples, seed, ao_mint, ao_maxt, accel, ao.as_mut_ptr(),
                                      std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut()) })?;
        Ok(ao)
    }
    /// Rust2's `Viewport::depth_map` in one launch, for a camera of `rtw_camera2_new`: row-major [height][width] hit.t, maxt * 1.6 on a
    /// miss (row j is row j of the image: the reference's leading empty row is not reproduced).
    pub fn depth_map(&mut self, cam: &RtwCamera, width: u32, height: u32, time: f32, mint: f32, maxt: f32, accel: u32) -> Result<Vec<f32>, RtwError> {
        let mut d = vec![0f32; width as usize * height as usize];
        check(unsafe { rtw_ctx_depth_map(self.ctx, cam, width, height, time, mint, maxt, accel, d.as_mut_ptr(), std::ptr::null_mut(),
                                         std::ptr::null_mut(), std::ptr::null_mut()) })?;
        Ok(d)
    }
    /// PerlinNoise::noise (turb_depth 0) / turb(p, turb_depth) at `points` on this context's GPU.
    pub fn perlin_eval(&mut self, t: &RtwPerlin, points: &[[f32; 3]], turb_depth: u32) -> Result<Vec<f32>, RtwError> {
        let mut out = vec![0f32; points.len()];
        check(unsafe { rtw_ctx_perlin_eval(self.ctx, t, points.as_ptr() as *const f32, points.len() as u32, turb_depth, out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// For tests: one of the hot path's arithmetic sequences (`RTW_MATH_*`) on this context's GPU, element i by thread i; `input` is
    /// [n][columns read], the result [n][columns written].
    pub fn device_math(&mut self, func: (u32, u32, u32), input: &[f32]) -> Result<Vec<f32>, RtwError> {
        let n = input.len() / func.1 as usize;
        let mut out = vec![0f32; n * func.2 as usize];
        check(unsafe { rtw_ctx_device_math(self.ctx, func.0, input.as_ptr(), func.1, n as u32, out.as_mut_ptr(), func.2) })?;
        Ok(out)
    }
    /// For tests: sqrt_plain / div_plain over `count` generated arguments from index `first`, each judged exactly on the GPU (`RTW_SWEEP_*`).
    pub fn device_sweep(&mut self, which: u32, first: u64, count: u64, seed: u32) -> Result<RtwSweepResult, RtwError> {
        let mut r = RtwSweepResult::default();
        check(unsafe { rtw_ctx_device_sweep(self.ctx, which, first, count, seed, &mut r) })?;
        Ok(r)
    }
    /// Rust2 `bilateral_filter` on this context's GPU: `rgb` is [h][w][3] u8 (`ImageBuffer<Rgb<u8>>::as_raw()`) or, with
    /// in_format 1, the f32 frame of `render` flattened; bit-identical to the reference.
    pub fn bilateral_filter(&mut self, rgb: *const c_void, w: u32, h: u32, p: &RtwBilateral) -> Result<(Vec<u8>, RtwFilterStats), RtwError> {
        let mut out = vec![0u8; w as usize * h as usize * 3];
        let mut st = RtwFilterStats::default();
        check(unsafe { rtw_ctx_bilateral_filter(self.ctx, rgb, w, h, p, out.as_mut_ptr(), &mut st) })?;
        Ok((out, st))
    }
    /// The guided filter on this context's GPU (rtw_ctx_guided_filter): `bilateral_filter` with every tap weighted by the guides -- depth
    /// [h][w] f32, normal [h][w][3] f32, idx [h][w] i32, each host or device memory, null where its term is off.
    pub fn guided_filter(&mut self, rgb: *const c_void, w: u32, h: u32, depth: *const f32, normal: *const f32, idx: *const i32,
                         p: &RtwGuidedFilter) -> Result<(Vec<u8>, RtwFilterStats), RtwError> {
        let mut out = vec![0u8; w as usize * h as usize * 3];
        let mut st = RtwFilterStats::default();
        check(unsafe { rtw_ctx_guided_filter(self.ctx, rgb, w, h, depth, normal, idx, p, out.as_mut_ptr(), &mut st) })?;
        Ok((out, st))
    }
    /// The a-trous filter on this context's GPU (rtw_ctx_atrous_filter): a linear f32 frame [h][w][3], the guides of `guided_filter`, albedo
    /// and emitted [h][w][3] f32; each host or device memory, null where its term is off or it is not given.
    pub fn atrous_filter(&mut self, rgb: *const f32, w: u32, h: u32, depth: *const f32, normal: *const f32, idx: *const i32, albedo: *const f32,
                         emitted: *const f32, p: &RtwAtrous) -> Result<(Vec<f32>, RtwFilterStats), RtwError> {
        let mut out = vec![0f32; w as usize * h as usize * 3];
        let mut st = RtwFilterStats::default();
        check(unsafe { rtw_ctx_atrous_filter(self.ctx, rgb, w, h, depth, normal, idx, albedo, emitted, p, out.as_mut_ptr(), &mut st) })?;
        Ok((out, st))
    }
    /// The variance estimate on this context's GPU (rtw_ctx_variance_estimate): moments [h][w][2] and len [h][w] as the temporal
    /// accumulation writes them, the guides of `atrous_filter`; each host or device memory, a guide null where its term is off.
    pub fn variance_estimate(&mut self, moments: *const f32, len: *const f32, w: u32, h: u32, depth: *const f32, normal: *const f32,
                             idx: *const i32, p: &RtwVarianceEstimate) -> Result<(Vec<f32>, RtwFilterStats), RtwError> {
        let mut out = vec![0f32; w as usize * h as usize];
        let mut st = RtwFilterStats::default();
        check(unsafe { rtw_ctx_variance_estimate(self.ctx, moments, len, w, h, depth, normal, idx, p, out.as_mut_ptr(), &mut st) })?;
        Ok((out, st))
    }
    /// The temporal accumulation on this context's GPU with moving objects (rtw_ctx_temporal_accumulate_motion): `rows` (may be null: the
    /// world is static) holds the motion of the objects surface_map reports as first .. first + n_rows - 1; prev_cam None on a first frame.
    #[allow(clippy::too_many_arguments)]
    pub fn temporal_accumulate_motion(&mut self, b: &TemporalBuffers, w: u32, h: u32, cam: &RtwCamera, prev_cam: Option<&RtwCamera>, p: &RtwTemporal,
                                      rows: *const RtwMotionRow, n_rows: u32, first: u32) -> Result<RtwFilterStats, RtwError> {
        let mut st = RtwFilterStats::default();
        let pc = prev_cam.map_or(std::ptr::null(), |c| c as *const RtwCamera);
        check(unsafe { rtw_ctx_temporal_accumulate_motion(self.ctx, b.cur, w, h, cam, b.depth, b.normal, b.idx, pc, b.prev_color, b.prev_moments,
                                                          b.prev_len, b.prev_depth, b.prev_normal, b.prev_idx, p, rows, n_rows, first, b.out_color,
                                                          b.out_moments, b.out_len, b.out_variance, b.out_prev_xy, &mut st) })?;
        Ok(st)
    }
    /// The motion rows of mesh placements on this context's GPU (rtw_ctx_mesh_instance_motion): poses [n][7] and rows_out [n], each host
    /// or device memory; returns the number of refused poses.
    pub fn mesh_instance_motion(&mut self, prev: *const f32, cur: *const f32, n: u32, rows_out: *mut RtwMotionRow) -> Result<u32, RtwError> {
        let mut bad = 0u32;
        check(unsafe { rtw_ctx_mesh_instance_motion(self.ctx, prev, cur, n, rows_out, &mut bad) })?;
        Ok(bad)
    }
    /// The variance-steered a-trous filter on this context's GPU (rtw_ctx_svgf_filter): `atrous_filter`'s arguments and a variance
    /// [h][w] f32; returns the filtered frame, the filtered variance and the stats.
    #[allow(clippy::type_complexity)]
    pub fn svgf_filter(&mut self, rgb: *const f32, variance: *const f32, w: u32, h: u32, depth: *const f32, normal: *const f32, idx: *const i32,
                       albedo: *const f32, emitted: *const f32, p: &RtwAtrous, vp: &RtwSvgf) -> Result<(Vec<f32>, Vec<f32>, RtwFilterStats), RtwError> {
        let n = w as usize * h as usize;
        let (mut out, mut var) = (vec![0f32; 3 * n], vec![0f32; n]);
        let mut st = RtwFilterStats::default();
        check(unsafe { rtw_ctx_svgf_filter(self.ctx, rgb, variance, w, h, depth, normal, idx, albedo, emitted, p, vp, out.as_mut_ptr(),
                                           var.as_mut_ptr(), &mut st) })?;
        Ok((out, var, st))
    }
    /// What a camera sees (rtw_ctx_surface_map): (depth, idx, normal, albedo, emitted, material) of every pixel's first surface under
    /// `integrator`, rays by `ray_rule` (`RTW_RAYS_PIXEL` with `offset` inside the pixel for Viewport cameras).
    #[allow(clippy::type_complexity)]
    pub fn surface_map(&mut self, cam: &RtwCamera, width: u32, height: u32, ray_rule: u32, offset: [f32; 2], time: f32, mint: f32, maxt: f32,
                       accel: u32, integrator: u32) -> Result<(Vec<f32>, Vec<i32>, Vec<f32>, Vec<f32>, Vec<f32>, Vec<f32>), RtwError> {
        let n = width as usize * height as usize;
        let (mut d, mut i) = (vec![0f32; n], vec![0i32; n]);
        let (mut nr, mut al, mut em, mut mt) = (vec![0f32; 3 * n], vec![0f32; 3 * n], vec![0f32; 3 * n], vec![0f32; 3 * n]);
        check(unsafe { rtw_ctx_surface_map(self.ctx, cam, width, height, ray_rule, offset.as_ptr(), time, mint, maxt, accel, integrator,
                                           d.as_mut_ptr(), i.as_mut_ptr(), nr.as_mut_ptr(), al.as_mut_ptr(), em.as_mut_ptr(), mt.as_mut_ptr(),
                                           std::ptr::null_mut()) })?;
        Ok((d, i, nr, al, em, mt))
    }
    /// rtw_ctx_scene_surface: `scene_hits` with albedo, emitted and material of each ray's first surface ([n][6] rays).
    #[allow(clippy::type_complexity)]
    pub fn scene_surface(&mut self, rays: &[[f32; 6]], time: f32, mint: f32, maxt: f32, accel: u32, integrator: u32)
                         -> Result<(Vec<f32>, Vec<i32>, Vec<f32>, Vec<f32>, Vec<f32>, Vec<f32>), RtwError> {
        let n = rays.len();
        let (mut t, mut i) = (vec![0f32; n], vec![0i32; n]);
        let (mut nr, mut al, mut em, mut mt) = (vec![0f32; 3 * n], vec![0f32; 3 * n], vec![0f32; 3 * n], vec![0f32; 3 * n]);
        check(unsafe { rtw_ctx_scene_surface(self.ctx, rays.as_ptr() as *const f32, n as u32, time, mint, maxt, accel, integrator, t.as_mut_ptr(),
                                             i.as_mut_ptr(), nr.as_mut_ptr(), al.as_mut_ptr(), em.as_mut_ptr(), mt.as_mut_ptr(),
                                             std::ptr::null_mut()) })?;
        Ok((t, i, nr, al, em, mt))
    }
    /// Tuning knobs (`RTW_OPT_*` of rtw.h: 1 chunk length, 2 sample bank GiB, 3 LDS geometry, 4 workgroups per CU, 5 list-walk
    /// threshold, 11 = `RTW_OPT_NODE_FORMAT`: the tree in LDS as 0 f32 planes where they fit, 1 f16 nodes, 2 f32 planes, 12 =
    /// `RTW_OPT_MESH_LIST_MAX`: at most this many mesh placements are met in list order, more through the top-level tree); none of them
    /// changes the image.
    pub fn set_option(&mut self, key: u32, value: f64) -> Result<(), RtwError> { check(unsafe { rtw_ctx_set_option(self.ctx, key, value) }) }
    /// The format of the tree the last render's kernel read from LDS (rtw_ctx_last_node_format): 0 none, 1 f16 nodes, 2 f32 planes.
    pub fn last_node_format(&mut self) -> Result<u32, RtwError> {
        let rc = unsafe { rtw_ctx_last_node_format(self.ctx) };
        if rc < 0 { check(rc)?; }
        Ok(rc as u32)
    }
    /// -> `Img`-shaped rows ([height][width] of Rgb<f32>), gamma-corrected, unclamped (viewport.rs:301).
    pub fn render(&mut self, cam: &RtwCamera, p: &RtwParams) -> Result<(Vec<Vec<[f32; 3]>>, RtwStats), RtwError> {
        // a row partition (RtwParams.part_count > 1) returns only the rows it owns, compactly
        let rows = unsafe { rtw_part_rows(p.height, p.row_block, p.part_index, p.part_count) } as usize;
        let mut flat = vec![[0f32; 3]; (p.width as usize) * rows];
        let mut st = RtwStats::default();
        check(unsafe { rtw_ctx_render(self.ctx, cam, p, flat.as_mut_ptr() as *mut c_void, &mut st) })?;
        let rows = flat.chunks(p.width as usize).take(st.rows as usize).map(|r| r.to_vec()).collect();
        Ok((rows, st))
    }
}
impl Renderer {
    /// == `render_multi` (viewport.rs:249-269): frames start_frame .. start_frame + n_frames at time frame / fps.
    pub fn render_multi(&mut self, cam: &RtwCamera, p: &RtwParams, fps: f32, start_frame: u32, n_frames: u32)
        -> Result<Vec<Vec<Vec<[f32; 3]>>>, RtwError> {
        let per = (p.width as usize) * (p.height as usize);
        let mut flat = vec![[0f32; 3]; per * n_frames as usize];
        check(unsafe { rtw_ctx_render_multi(self.ctx, cam, p, fps, start_frame, n_frames, flat.as_mut_ptr() as *mut c_void, std::ptr::null_mut()) })?;
        Ok(flat.chunks(per).map(|f| f.chunks(p.width as usize).map(|r| r.to_vec()).collect()).collect())
    }
}
impl Drop for Renderer { fn drop(&mut self) { unsafe { rtw_ctx_destroy(self.ctx) } } }

/// All GPUs of a node from one host thread: the fork / ordered join of `async_render`'s row tasks
/// (viewport.rs:236-244; rayon: Rust2/src/viewport.rs:119-122) with GPUs in place of worker threads.  The host owns the
/// frame (`Img`); every GPU copies its interleaved 8-row blocks straight into their image rows.
pub struct MultiRenderer { m: *mut RtwMgpu, n: usize }
impl MultiRenderer {
    pub fn new(devices: &[i32]) -> Result<Self, RtwError> {
        let mut m = std::ptr::null_mut();
        check(unsafe { rtw_mgpu_create(devices.as_ptr(), devices.len() as u32, &mut m) })?;
        Ok(Self { m, n: devices.len() })
    }
    pub fn set_scene(&mut self, sc: &RtwScene, t_begin: f32, t_end: f32) -> Result<(), RtwError> {
        check(unsafe { rtw_mgpu_set_scene(self.m, sc, t_begin, t_end) })
    }
    /// rtw_mgpu_set_instance_rotations: `Renderer::set_instance_rotations` on every device.
    pub fn set_instance_rotations(&mut self, quats: &[[f32; 4]]) -> Result<(), RtwError> {
        let p = if quats.is_empty() { std::ptr::null() } else { quats.as_ptr() };
        check(unsafe { rtw_mgpu_set_instance_rotations(self.m, p, quats.len() as u32) })
    }
    /// rtw_mgpu_set_mesh_instances: `Renderer::set_mesh_instances` on every device.
    pub fn set_mesh_instances(&mut self, placements: &[RtwMeshInstance]) -> Result<(), RtwError> {
        let p = if placements.is_empty() { std::ptr::null() } else { placements.as_ptr() };
        check(unsafe { rtw_mgpu_set_mesh_instances(self.m, p, placements.len() as u32) })
    }
    pub fn render(&mut self, cam: &RtwCamera, p: &RtwParams) -> Result<(Vec<Vec<[f32; 3]>>, Vec<RtwStats>), RtwError> {
        let mut flat = vec![[0f32; 3]; (p.width as usize) * (p.height as usize)];
        let mut per = vec![RtwStats::default(); self.n];
        check(unsafe { rtw_mgpu_render(self.m, cam, p, flat.as_mut_ptr() as *mut c_void, per.as_mut_ptr(), std::ptr::null_mut()) })?;
        Ok((flat.chunks(p.width as usize).map(|r| r.to_vec()).collect(), per))
    }
}
impl Drop for MultiRenderer { fn drop(&mut self) { unsafe { rtw_mgpu_destroy(self.m) } } }

// In the reference crate, next to `impl Viewport` (viewport.rs:307):
//
// impl Viewport {
//     pub fn render_gpu(&self, ray_color: Integrator, scene: &Scene) -> Result<Img, RtwError> {
//         let cam = RtwCamera { origin: self.origin.into(), u: self.u.into(), v: self.v.into(),
//             pixel00: self.upper_left_corner.into(), delta_u: self.p_delta_u.into(), delta_v: self.p_delta_v.into(),
//             lens_radius: self.lens_radius, time0: self.frame as f32 / self.fps, shutter: self.shutter_speed };
//         let spheres: Vec<RtwSphere> = scene.spheres.iter().map(|s| RtwSphere {
//             center: s.origin.into(), radius: s.radius, velocity: s.velocity.into(), col_mod: s.col_mod.into(),
//             tex_color: /* 1x1 texel, or [1.;3] with tex = index */, metallicness: s.mat.metallicness,
//             opacity: s.mat.opacity, ir: s.mat.ir, emitted: s.mat.emmited.into(), tex: -1 }).collect();
//         let p = RtwParams { width: self.width as u32, height: self.height as u32, samples: self.samples as u32,
//             depth: self.depth as u32, gamma: self.gamma, mint: 0.001, maxt: 100000.0, integrator: ray_color as u32,
//             sampler: Sampler::Stratified as u32, accel: 1, flags: 0, seed: 1, row_block: 8, part_index: 0, part_count: 1, reserved: 0 };
//         let mut r = Renderer::new(0)?;
//         r.set_scene(&spheres, &[], &[], scene.background_color.into(), cam.time0, cam.time0 + cam.shutter)?;
//         Ok(r.render(&cam, &p)?.0.into_iter().map(|row| row.into_iter().map(Rgb).collect()).collect())
//     }
// }

impl RtwPerlin {
    /// PerlinNoise::new (texture.rs:110-149) with the tables drawn from PCG32(seed) (host only).
    pub fn new(seed: u64) -> Result<RtwPerlin, RtwError> {
        let mut t = RtwPerlin { ranvec: [[0.0; 3]; 256], perm_x: [0; 256], perm_y: [0; 256], perm_z: [0; 256] };
        check(unsafe { rtw_perlin_new(seed, &mut t) })?;
        Ok(t)
    }
    /// PerlinNoise::noise (turb_depth 0) / turb(p, turb_depth) on the host.
    pub fn eval(&self, points: &[[f32; 3]], turb_depth: u32) -> Result<Vec<f32>, RtwError> {
        let mut out = vec![0f32; points.len()];
        check(unsafe { rtw_perlin_eval(self, points.as_ptr() as *const f32, points.len() as u32, turb_depth, out.as_mut_ptr()) })?;
        Ok(out)
    }
}

/// rtw_mgpu_set_texture_noise: the same on every device of an `rtw_mgpu` (handle from rtw_mgpu_create).
pub unsafe fn mgpu_set_texture_noise(m: *mut RtwMgpu, tables: &[RtwPerlin], per_texture: &[RtwTextureNoise]) -> i32 {
    rtw_mgpu_set_texture_noise(m, tables.as_ptr(), tables.len() as u32, per_texture.as_ptr(), per_texture.len() as u32)
}

/// rtw_bilateral_filter: the library's host form of Rust2's `bilateral_filter` on a [h][w][3] u8 image.
pub fn bilateral_filter_host(rgb: &[u8], w: u32, h: u32, proximity: Proximity) -> Result<Vec<u8>, RtwError> {
    let p = RtwBilateral { size: proximity.size, proximity: proximity.kind as u32, in_format: 0, avg_gradient: 0.0 };
    let mut out = vec![0u8; rgb.len()];
    check(unsafe { rtw_bilateral_filter(rgb.as_ptr() as *const c_void, w, h, &p, out.as_mut_ptr(), std::ptr::null_mut()) })?;
    Ok(out)
}

/// rtw_guided_filter: the host form of the guided filter (a guide whose term is off may be empty).
pub fn guided_filter_host(rgb: &[u8], w: u32, h: u32, depth: &[f32], normal: &[f32], idx: &[i32], p: &RtwGuidedFilter) -> Result<Vec<u8>, RtwError> {
    let mut out = vec![0u8; rgb.len()];
    let ptr = |n: usize, q: *const c_void| if n == 0 { std::ptr::null() } else { q };
    check(unsafe { rtw_guided_filter(rgb.as_ptr() as *const c_void, w, h, ptr(depth.len(), depth.as_ptr() as *const c_void) as *const f32,
                                     ptr(normal.len(), normal.as_ptr() as *const c_void) as *const f32,
                                     ptr(idx.len(), idx.as_ptr() as *const c_void) as *const i32, p, out.as_mut_ptr(), std::ptr::null_mut()) })?;
    Ok(out)
}

/// rtw_atrous_filter: the host form of the a-trous filter (a guide whose term is off, albedo and emitted may be empty).
pub fn atrous_filter_host(rgb: &[f32], w: u32, h: u32, depth: &[f32], normal: &[f32], idx: &[i32], albedo: &[f32], emitted: &[f32],
                          p: &RtwAtrous) -> Result<Vec<f32>, RtwError> {
    let mut out = vec![0f32; rgb.len()];
    let f = |s: &[f32]| if s.is_empty() { std::ptr::null() } else { s.as_ptr() };
    let ids = if idx.is_empty() { std::ptr::null() } else { idx.as_ptr() };
    check(unsafe { rtw_atrous_filter(rgb.as_ptr(), w, h, f(depth), f(normal), ids, f(albedo), f(emitted), p, out.as_mut_ptr(), std::ptr::null_mut()) })?;
    Ok(out)
}

/// rtw_variance_estimate: the host form of the variance estimate (a guide whose term is off may be empty).
pub fn variance_estimate_host(moments: &[f32], len: &[f32], w: u32, h: u32, depth: &[f32], normal: &[f32], idx: &[i32],
                              p: &RtwVarianceEstimate) -> Result<Vec<f32>, RtwError> {
    let mut out = vec![0f32; len.len()];
    let f = |s: &[f32]| if s.is_empty() { std::ptr::null() } else { s.as_ptr() };
    let ids = if idx.is_empty() { std::ptr::null() } else { idx.as_ptr() };
    check(unsafe { rtw_variance_estimate(f(moments), f(len), w, h, f(depth), f(normal), ids, p, out.as_mut_ptr(), std::ptr::null_mut()) })?;
    Ok(out)
}

/// rtw_svgf_filter: the host form of the variance-steered a-trous filter, (frame, variance) (a guide whose term is off, albedo and emitted
/// may be empty).
#[allow(clippy::too_many_arguments)]
pub fn svgf_filter_host(rgb: &[f32], variance: &[f32], w: u32, h: u32, depth: &[f32], normal: &[f32], idx: &[i32], albedo: &[f32],
                        emitted: &[f32], p: &RtwAtrous, vp: &RtwSvgf) -> Result<(Vec<f32>, Vec<f32>), RtwError> {
    let (mut out, mut var) = (vec![0f32; rgb.len()], vec![0f32; variance.len()]);
    let f = |s: &[f32]| if s.is_empty() { std::ptr::null() } else { s.as_ptr() };
    let ids = if idx.is_empty() { std::ptr::null() } else { idx.as_ptr() };
    check(unsafe { rtw_svgf_filter(f(rgb), f(variance), w, h, f(depth), f(normal), ids, f(albedo), f(emitted), p, vp, out.as_mut_ptr(),
                                   var.as_mut_ptr(), std::ptr::null_mut()) })?;
    Ok((out, var))
}

/// rtw_pixel_rays: the pixel rays of a Viewport camera at `offset` inside the pixel, [h * w][6] = origin, direction (not normalised).
pub fn pixel_rays(cam: &RtwCamera, width: u32, height: u32, offset: [f32; 2]) -> Result<Vec<[f32; 6]>, RtwError> {
    let mut r = vec![[0f32; 6]; width as usize * height as usize];
    check(unsafe { rtw_pixel_rays(cam, width, height, offset.as_ptr(), r.as_mut_ptr() as *mut f32) })?;
    Ok(r)
}

/// Rust2 `bilateral_filter(img, proximity)` on GPU 0 for a [h][w][3] u8 image (`Img::as_raw()`), bit-identical to the reference.
impl RtwTriangle {
    /// Rust2 `Triangle::new(origin, u, v, mat, ConstColorTexture(color))` (tex = -1) or with `textures[tex]`.
    pub fn new(origin: [f32; 3], u: [f32; 3], v: [f32; 3], mat3: [f32; 3], emitted: [f32; 3], color: [f32; 3], tex: i32) -> Result<Self, RtwError> {
        let mut t = RtwTriangle::default();
        check(unsafe { rtw_triangle_new(origin.as_ptr(), u.as_ptr(), v.as_ptr(), mat3.as_ptr(), emitted.as_ptr(), color.as_ptr(), tex, &mut t) })?;
        Ok(t)
    }
}

/// The closest triangle per ray on the host (the list walk): (t, index or -1) per ray.
pub fn triangle_hits(tris: &[RtwTriangle], rays: &[[f32; 6]], mint: f32, maxt: f32) -> Result<(Vec<f32>, Vec<i32>), RtwError> {
    let (mut t, mut i) = (vec![0f32; rays.len()], vec![0i32; rays.len()]);
    check(unsafe { rtw_triangle_hits(tris.as_ptr(), tris.len() as u32, rays.as_ptr() as *const f32, rays.len() as u32, mint, maxt,
                                     t.as_mut_ptr(), i.as_mut_ptr()) })?;
    Ok((t, i))
}

/// rtw_mesh_instances_validate: the status rtw_ctx_set_mesh_instances answers for `placements` of the mesh `tris` (host only).
pub fn mesh_instances_validate(tris: &[RtwTriangle], placements: &[RtwMeshInstance]) -> i32 {
    let t = if tris.is_empty() { std::ptr::null() } else { tris.as_ptr() };
    let p = if placements.is_empty() { std::ptr::null() } else { placements.as_ptr() };
    unsafe { rtw_mesh_instances_validate(t, tris.len() as u32, p, placements.len() as u32) }
}

/// The motion rows of mesh placements that went from `prev` to `cur` (rtw_mesh_instance_motion, host only): poses of position xyz,
/// quaternion wxyz; returns the rows and the number of refused poses.
pub fn mesh_instance_motion(prev: &[[f32; 7]], cur: &[[f32; 7]]) -> Result<(Vec<RtwMotionRow>, u32), RtwError> {
    assert_eq!(prev.len(), cur.len());
    let mut rows = vec![RtwMotionRow::default(); cur.len()];
    let mut bad = 0u32;
    check(unsafe { rtw_mesh_instance_motion(prev.as_ptr() as *const f32, cur.as_ptr() as *const f32, cur.len() as u32, rows.as_mut_ptr(), &mut bad) })?;
    Ok((rows, bad))
}

/// rtw_temporal_accumulate_motion: the host form of `Renderer::temporal_accumulate_motion`, host memory only.
#[allow(clippy::too_many_arguments)]
pub fn temporal_accumulate_motion_host(b: &TemporalBuffers, w: u32, h: u32, cam: &RtwCamera, prev_cam: Option<&RtwCamera>, p: &RtwTemporal,
                                       rows: &[RtwMotionRow], first: u32) -> Result<RtwFilterStats, RtwError> {
    let mut st = RtwFilterStats::default();
    let pc = prev_cam.map_or(std::ptr::null(), |c| c as *const RtwCamera);
    let r = if rows.is_empty() { std::ptr::null() } else { rows.as_ptr() };
    check(unsafe { rtw_temporal_accumulate_motion(b.cur, w, h, cam, b.depth, b.normal, b.idx, pc, b.prev_color, b.prev_moments, b.prev_len,
                                                  b.prev_depth, b.prev_normal, b.prev_idx, p, r, rows.len() as u32, first, b.out_color, b.out_moments,
                                                  b.out_len, b.out_variance, b.out_prev_xy, &mut st) })?;
    Ok(st)
}

/// The closest placement of the mesh per ray on the host (rtw_mesh_instance_hits, the list walk).
pub fn mesh_instance_hits(tris: &[RtwTriangle], placements: &[RtwMeshInstance], rays: &[[f32; 6]], mint: f32, maxt: f32) -> Result<MeshHits, RtwError> {
    let n = rays.len();
    let (mut t, mut p, mut i, mut nr) = (vec![0f32; n], vec![0i32; n], vec![0i32; n], vec![[0f32; 3]; n]);
    check(unsafe { rtw_mesh_instance_hits(tris.as_ptr(), tris.len() as u32, placements.as_ptr(), placements.len() as u32, rays.as_ptr() as *const f32,
                                          n as u32, mint, maxt, t.as_mut_ptr(), p.as_mut_ptr(), i.as_mut_ptr(), nr.as_mut_ptr() as *mut f32) })?;
    Ok((t, p, i, nr))
}

/// Rust2's `Camera::new(aspect, origin, vup, dir, vfov, lens_radius)` (Rust2/src/viewport/camera.rs:19-53).
pub fn camera2_new(aspect: f32, origin: [f32; 3], vup: [f32; 3], dir: [f32; 3], vfov: f32, lens_radius: f32) -> Result<RtwCamera, RtwError> {
    let mut cam = RtwCamera::default();
    check(unsafe { rtw_camera2_new(aspect, origin.as_ptr(), vup.as_ptr(), dir.as_ptr(), vfov, lens_radius, &mut cam) })?;
    Ok(cam)
}

/// Rust2's `Quaternion::rotate` ([w, x, y, z]; q need not be normalised), the definition the kernels compile (host only).
pub fn quat_rotate(q: [f32; 4], v: [f32; 3]) -> [f32; 3] {
    let mut out = [0f32; 3];
    unsafe { rtw_quat_rotate(q.as_ptr(), v.as_ptr(), out.as_mut_ptr()) };
    out
}
/// `a.hamilton(&b)`: `Instance::rotate(rot)` is `rotation = quat_mul(rotation, rot)`.
pub fn quat_mul(a: [f32; 4], b: [f32; 4]) -> [f32; 4] {
    let mut out = [0f32; 4];
    unsafe { rtw_quat_mul(a.as_ptr(), b.as_ptr(), out.as_mut_ptr()) };
    out
}
/// `Quaternion::new_from_axis(angle, axis)`.
pub fn quat_from_axis(angle: f32, axis: [f32; 3]) -> [f32; 4] {
    let mut out = [0f32; 4];
    unsafe { rtw_quat_from_axis(angle, axis.as_ptr(), out.as_mut_ptr()) };
    out
}
/// `Quaternion::from(&EulerAngles { x, y, z })`.
pub fn quat_from_euler(euler: [f32; 3]) -> [f32; 4] {
    let mut out = [0f32; 4];
    unsafe { rtw_quat_from_euler(euler.as_ptr(), out.as_mut_ptr()) };
    out
}

/// The rays of ambient occlusion (host only): `samples` [origin, direction] per point, point-major; six zeros for a skipped point's.
pub fn ao_rays(points: &[[f32; 3]], normals: &[[f32; 3]], samples: u32, seed: u32) -> Result<Vec<[f32; 6]>, RtwError> {
    if points.len() != normals.len() || samples == 0 || samples > 1024 { return Err(RtwError(-1)); }
    let mut r = vec![[0f32; 6]; points.len() * samples as usize];
    check(unsafe { rtw_ao_rays(points.as_ptr() as *const f32, normals.as_ptr() as *const f32, points.len() as u32, samples, seed,
                               r.as_mut_ptr() as *mut f32) })?;
    Ok(r)
}

/// The rays of Rust2's `Viewport::depth_map` for a camera of `rtw_camera2_new` (host only): [origin, unit direction] per pixel, row-major.
pub fn depth_rays(cam: &RtwCamera, width: u32, height: u32) -> Result<Vec<[f32; 6]>, RtwError> {
    let mut r = vec![[0f32; 6]; width as usize * height as usize];
    check(unsafe { rtw_depth_rays(cam, width, height, r.as_mut_ptr() as *mut f32) })?;
    Ok(r)
}

pub fn bilateral_filter_gpu(rgb: &[u8], w: u32, h: u32, proximity: Proximity) -> Result<Vec<u8>, RtwError> {
    let p = RtwBilateral { size: proximity.size, proximity: proximity.kind as u32, in_format: 0, avg_gradient: 0.0 };
    Ok(Renderer::new(0)?.bilateral_filter(rgb.as_ptr() as *const c_void, w, h, &p)?.0)
}

// In the reference crate (Rust2/src/postprocessing.rs, next to `bilateral_filter`), with its `Img` type:
//
// pub(crate) fn bilateral_filter_gpu(img: &Img, proximity: Proximity) -> Result<Img, RtwError> {
//     let (w, h) = img.dimensions();
//     let raw = rtw::bilateral_filter_gpu(img.as_raw(), w, h, proximity)?;
//     Ok(ImageBuffer::from_raw(w, h, raw).unwrap())
// }

/// Host only, for tests: is got[i] the correctly rounded f32 sqrt(a[i]) (`RTW_SWEEP_SQRT`, `b` unused) or a[i] / b[i]?  Bit patterns.
pub fn rounding_check(which: u32, a: &[u32], b: &[u32], got: &[u32]) -> Result<Vec<bool>, RtwError> {
    let mut ok = vec![0u8; a.len()];
    let bp = if b.is_empty() { std::ptr::null() } else { b.as_ptr() };
    check(unsafe { rtw_rounding_check(which, a.as_ptr(), bp, got.as_ptr(), a.len(), ok.as_mut_ptr()) })?;
    Ok(ok.into_iter().map(|v| v != 0).collect())
}
/// Host only, for tests: the (n, d) bit patterns a quotient sweep forms for indices first .. first + n - 1.
pub fn sweep_operands(which: u32, first: u64, n: usize, seed: u32) -> Result<Vec<[u32; 2]>, RtwError> {
    let mut out = vec![[0u32; 2]; n];
    check(unsafe { rtw_sweep_operands(which, first, n, seed, out.as_mut_ptr() as *mut u32) })?;
    Ok(out)
}
