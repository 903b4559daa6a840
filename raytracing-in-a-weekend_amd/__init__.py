"""rtw-mi355x: MI355X-native path tracer behind the reference's Viewport/Scene/Sphere/Material surface.

This package is a thin ctypes binding over ``librtw_hip.so`` (the product: hand-written HIP kernels
for gfx950 + the C ABI of ``include/rtw.h`` + the C++ host mirror of the reference constructors).
Python only moves pointers; it does no arithmetic on the render path, and there is NO CPU fallback:
if the HIP library is missing or no GPU is present, rendering raises.

Reference surface mirrored (names and argument meaning):
  Viewport.new_from_res / Viewport.new      Rust/src/viewport.rs:308-428
  Viewport.render / async_render            Rust/src/viewport.rs:215-248,430-478
  Scene.new_sphere                          Rust/src/viewport.rs:90-105
  Scene.new / new_quad                      Rust/src/viewport.rs:106-135
  Sphere.new / new_moving / new_with_texture Rust/src/objects/sphere.rs:151-247
  Quad.new                                  Rust/src/objects/quad.rs:84-110
  Instance.new / new_quads / new_sphere / new_box, translate, rotate   Rust/src/objects/instance.rs:83-248
  METALLIC_M, SCATTER_M, FUZZY3_M, GLASS_M, GLASSR_M   Rust/src/objects/materials.rs:157-212
  PerlinNoise.new / noise / turb / value    Rust/src/texture.rs:61-194
  ImageTexture::from_color_noise / new_with_noise      Rust/src/texture.rs:228-245 (texture_from_color_noise, texture_with_noise)
  bilateral_filter(img, Proximity::new(size, type))  Rust2/src/postprocessing.rs:12-131 (bilateral_filter; Renderer.bilateral_filter)
  (extension) guided_filter(img, size, depth=, normal=, ids=, ..)   the bilateral filter steered by depth_map's buffers (Renderer.guided_filter)
  (extension) atrous_filter(frame, depth=, normal=, ids=, albedo=, emitted=, ..)   an edge-avoiding a-trous wavelet filter of linear f32 frames (Renderer.atrous_filter)
  (extension) temporal_accumulate(cur, cam, depth=, normal=, ids=, history=, ..)   frames of a sequence blended along reprojected pixels (Renderer.temporal_accumulate, TemporalDenoiser)
  (extension) temporal_accumulate(.., motion=, motion_first=, out_prev_xy=)        ... with objects that moved rigidly since the previous frame (mesh_instance_motion, motion_rows)
  (extension) colour_bounds(frame, ids=, radius=, k=, ..)   mean +- k sigma of the frame around each pixel: the firefly clamp, and the box of temporal_accumulate(.., hist_lo=, hist_hi=) (Renderer.colour_bounds)
  (extension) variance_estimate(moments, length, depth=, normal=, ids=, ..)   a luminance variance for every pixel of an accumulated frame (Renderer.variance_estimate)
  (extension) svgf_filter(frame, variance, depth=, normal=, ids=, albedo=, emitted=, ..)   the a-trous filter steered by that variance (Renderer.svgf_filter, SvgfDenoiser)
  Triangle.new (+ from_mesh), Scene(triangles=)       Rust2/src/objects/triangle.rs:28-124 (triangle_hits; Renderer.triangle_hits)

The directory name carries a hyphen (it is fixed by the build contract); import it with
``importlib.import_module("raytracing-in-a-weekend_amd")`` or through the ``rtw_amd`` alias module
at the repo root.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTW_HIP_LIB", os.path.join(_HERE, "librtw_hip.so"))   # override: A/B builds of the same ABI

# ---- enums (include/rtw.h) ---------------------------------------------------------------------
RTW_OK = 0
INTEGRATOR_GRADIENT, INTEGRATOR_BG_COLOR, INTEGRATOR_NORMAL, INTEGRATOR_FLAG, INTEGRATOR_RUST2 = 0, 1, 2, 3, 4
INTEGRATOR_LIGHT_CAST, INTEGRATOR_LIGHT_BIASED = 5, 6   # Rust2 light_biased_ray_cast / light_biased_ray_color (set_lights)
LIGHT_SPHERE, LIGHT_QUAD = 0, 1                         # RtwLight.kind
MAX_LIGHTS = 16
MAX_MESH_INSTANCES = 65536
SAMPLER_ROW, SAMPLER_STRATIFIED, SAMPLER_CENTRES, SAMPLER_NO_RAND = 0, 1, 2, 3
ACCEL_BRUTE, ACCEL_BVH = 0, 1
RAYS_DEPTH_MAP, RAYS_PIXEL = 0, 1                       # Renderer.surface_map's ray rule: depth_rays' (camera2_new) or pixel_rays' (Viewport cameras)
FLAG_RECURSIVE_ORDER, FLAG_CPP_DIELECTRIC, FLAG_GLOBAL_NODES, FLAG_CPP_DIFFUSE, FLAG_CHUNK_SUMS = 1, 2, 4, 8, 16
FLAG_CPP = FLAG_CPP_DIELECTRIC | FLAG_CPP_DIFFUSE      # what Viewport::RenderGPU of the C++ tree asks for
FLAG_MIXED_MATERIAL = 32   # Rust2's integrators: an object with opacity < 0 is MixedMaterial::new(ir) (see mixed())
OPT_CHUNK_LEN, OPT_SAMPLE_BANK_GB, OPT_LDS_GEOM, OPT_BLOCKS_PER_CU, OPT_LIST_WALK_MAX, OPT_TILE_ORDER, OPT_GRAB_BLOCKS, OPT_SUB_QUEUES = 1, 2, 3, 4, 5, 6, 7, 8
OPT_TAIL_UNITS = 9
OPT_NODE_FORMAT = 11                                 # the large-workgroup BVH builds' tree in LDS: 0 f32 planes where they fit, 1 f16 nodes, 2 f32 planes
NODE_FORMAT_NONE, NODE_FORMAT_F16, NODE_FORMAT_F32 = 0, 1, 2   # Renderer.last_node_format
OPT_MESH_CLIMB = 13                                   # how move_mesh_instances climbs the top-level tree: 0 by node count, 1 per height, 2 one workgroup
OPT_MESH_LIST_MAX = 12                               # at most this many mesh placements: list order even under ACCEL_BVH; more: the top-level tree
MESH_LIST_MAX_DEFAULT = 16                           # its default (csrc/rtw_kernels.h RTW_MESH_LIST_MAX_DEFAULT): the measured crossover, DESIGN.md 4.11
OPT_GUIDED_LAYOUT = 10                               # Renderer.guided_filter: 0 by size, 1 table + guides in LDS, 2 guides, 3 table, 4 neither
OPT_HISTOGRAM_COUNT = 15                             # Renderer.luminance_histogram's LDS counts: 0 the measured choice, 1 plain, 2 per wave, 3 ballot
OPT_ATROUS_LAYOUT = 14                               # Renderer.atrous_filter: 0 the measured choice per level, 1 LDS tile where it fits, 2 global memory
ATROUS_MAX_LEVELS = 8
SCENE_C1, SCENE_C2, SCENE_C4, SCENE_C5, SCENE_METAL_TEST, SCENE_QUAD_TEST, SCENE_PRESENTATION, SCENE_FIRST_FRAME = 1, 2, 4, 5, 6, 7, 8, 9
MEDIUM_SURFACE, MEDIUM_CONST_DENSITY = 0, 1
PROXIMITY_SQUARE, PROXIMITY_EDGES = 0, 1             # Rust2 ProximityType (postprocessing.rs:12-15)
PIXELS_U8, PIXELS_F32_RUST2 = 0, 1                   # RtwBilateral.in_format
BILATERAL_MAX_SIZE = 64
STREAM_LEGACY = 1                                    # RTW_STREAM_LEGACY: HIP's legacy default stream, the one torch calls its default stream

# Renderer.atrous_filter's defaults: the best row, with albedo and emission, of the sweep on the 4-spp Book-1 view (profiles/atrous.log)
TEMPORAL_MAX_SIDE = 65535
# Renderer.temporal_accumulate's defaults: the best row, by the accumulated colour, of the sweep on the 4-spp Book-1 orbit (DESIGN.md 8d,
# profiles/temporal.log); max_history and same_object were not swept
TEMPORAL_DEFAULTS = {"alpha": 0.1, "alpha_moments": 0.1, "max_history": 32, "depth_tol": 0.05, "normal_cos": 0.9, "same_object": 1}
ATROUS_DEFAULTS = {"levels": 3, "sigma_color": 1.0, "sigma_depth": 0.25, "sigma_normal": 0.3, "albedo_floor": 1e-3}
VARIANCE_MAX_RADIUS = 3
# Renderer.variance_estimate's, Renderer.svgf_filter's and SvgfDenoiser's defaults: levels, sigma_luminance, min_history and prefilter are the
# best row, by the orbit's mean over frames 8..15, of the sweep on the 4-spp Book-1 orbit (profiles/svgf.log); the guide
# sigmas and the floor are the a-trous filter's, sigma_color is off, radius and epsilon were not swept
SVGF_DEFAULTS = {"levels": 3, "sigma_luminance": 1.0, "epsilon": 1e-8, "prefilter": False, "min_history": 4, "radius": 3, "sigma_color": 0.0,
                 "sigma_depth": ATROUS_DEFAULTS["sigma_depth"], "sigma_normal": ATROUS_DEFAULTS["sigma_normal"],
                 "albedo_floor": ATROUS_DEFAULTS["albedo_floor"]}
BOUNDS_MAX_RADIUS = 3
# Renderer.colour_bounds' defaults, and what to give firefly= / history_clamp= of the denoisers' steps: the row of the sweep with the least
# mean ratio, with both on, over the late frames of the five recorded sequences (0.359 against 0.400 as recorded; it helps four of them and
# costs on the light scene: DESIGN.md 8h, profiles/history_clamp.log).  The denoisers' own default stays None.
BOUNDS_DEFAULTS = {"radius": 1, "k": 1.0}
UPSAMPLE_MAX_SCALE = 8
UPSAMPLE_MAX_RADIUS = 2
# Renderer.upsample_filter's defaults: the best row of the sweep at half size on the 16-spp Book-1 view, by the sum of the upsampled and the
# filtered-then-upsampled column (profiles/upsample.log) -- the 4 x 4 tent, a tight normal term, same_object, no depth term.
# The a-trous filter's own sigmas (depth 0.25, normal 0.3) lose there: they let taps across a silhouette through, whose demodulated colour
# is wrong by the ratio of two albedos.
UPSAMPLE_DEFAULTS = {"radius": 2, "sigma_depth": 0.0, "sigma_normal": 0.1, "same_object": True, "albedo_floor": ATROUS_DEFAULTS["albedo_floor"]}
# The display stage (include/rtw.h "display stage")
TONE_NONE, TONE_REINHARD, TONE_REINHARD_LUMA, TONE_ACES_FIT = 0, 1, 2, 3
TRANSFER_GAMMA, TRANSFER_SRGB = 0, 1
QUANTISE_RUST, QUANTISE_RUST2 = 0, 1
DISPLAY_RGB8, DISPLAY_RGBA8, DISPLAY_F32 = 0, 1, 2
HISTOGRAM_BLOCKS_PER_CU = 4                           # Renderer.luminance_histogram's grid: at most this many workgroups a compute unit,
HISTOGRAM_BLOCK_PIXELS = 1024                         # each pass of a workgroup taking this many pixels
# display's defaults: exposure 1, the ACES fit (it needs no white point), sRGB, write_img_f32's byte rule, no dither, RGB8.  A choice, not a
# measurement: nothing here was tuned against anything.
DISPLAY_DEFAULTS = {"exposure": 1.0, "tone": TONE_ACES_FIT, "white": 4.0, "transfer": TRANSFER_SRGB, "gamma": 2.2, "quantise": QUANTISE_RUST,
                    "dither": False, "out_format": DISPLAY_RGB8}
# exposure_from_histogram's defaults: the darkest and brightest 5 % left out, middle grey, no adaptation, every level allowed.
METERING_DEFAULTS = {"low_permille": 50, "high_permille": 50, "key": 0.18, "rate": 1.0, "min_level": 0.0, "max_level": 256.0}
# Bloom (include/rtw.h "bloom")
BLOOM_MAX_LEVELS = 8
# bloom's defaults: six levels, the bright pass opening at luminance 1 with a knee of a half, the Karis weight on, a half of each coarser
# level on the way up, a quarter of the layer on the frame.  Choices, not measurements: nothing here was tuned against anything.
BLOOM_DEFAULTS = {"levels": 6, "threshold": 1.0, "knee": 0.5, "karis": True, "spread": 0.5, "intensity": 0.25}

# materials.rs:157-212 presets as (metallicness, opacity, ir)
METALLIC_M = (1.0, 0.0, 1.0)
SCATTER_M = (0.0, 0.0, 1.0)
FUZZY3_M = (0.7, 0.0, 1.0)
GLASS_M = (1.0, 1.0, 1.5)
GLASSR_M = (1.0, 1.0, float(np.float32(1.0) / np.float32(1.5)))
EMPTY_M = SCATTER_M


class RtwError(RuntimeError):
    def __init__(self, status: int, what: str):
        super().__init__(f"{what}: status {status} ({_strerror(status)})")
        self.status = status


# ---- PODs ----------------------------------------------------------------------------------------
class RtwCamera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3),
                ("pixel00", C.c_float * 3), ("delta_u", C.c_float * 3), ("delta_v", C.c_float * 3),
                ("lens_radius", C.c_float), ("time0", C.c_float), ("shutter", C.c_float)]


class RtwSphere(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("velocity", C.c_float * 3),
                ("col_mod", C.c_float * 3), ("tex_color", C.c_float * 3),
                ("metallicness", C.c_float), ("opacity", C.c_float), ("ir", C.c_float),
                ("emitted", C.c_float * 3), ("tex", C.c_int32)]


class RtwTexture(C.Structure):
    _fields_ = [("row", C.c_uint32), ("col", C.c_uint32), ("texel_offset", C.c_uint32), ("emit_tex", C.c_uint32)]


class RtwQuad(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3), ("velocity", C.c_float * 3),
                ("tex_color", C.c_float * 3), ("metallicness", C.c_float), ("opacity", C.c_float), ("ir", C.c_float),
                ("emitted", C.c_float * 3), ("tex", C.c_int32)]


class RtwTriangle(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3), ("normal", C.c_float * 3), ("d", C.c_float),
                ("w", C.c_float * 3), ("tex_color", C.c_float * 3), ("metallicness", C.c_float), ("opacity", C.c_float), ("ir", C.c_float),
                ("emitted", C.c_float * 3), ("tex", C.c_int32)]


class RtwMeshInstance(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("quat", C.c_float * 4)]


class RtwLight(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("index", C.c_uint32)]


class RtwInstance(C.Structure):
    _fields_ = [("first_sphere", C.c_uint32), ("n_spheres", C.c_uint32), ("first_quad", C.c_uint32), ("n_quads", C.c_uint32),
                ("translation", C.c_float * 3), ("rotation", C.c_float * 3), ("density", C.c_float), ("medium", C.c_uint32)]


class RtwScene(C.Structure):
    _fields_ = [("spheres", C.POINTER(RtwSphere)), ("textures", C.POINTER(RtwTexture)),
                ("texels", C.POINTER(C.c_float)), ("n_spheres", C.c_uint32), ("n_textures", C.c_uint32),
                ("n_texels", C.c_uint32), ("background", C.c_float * 3),
                ("quads", C.POINTER(RtwQuad)), ("instances", C.POINTER(RtwInstance)),
                ("inst_spheres", C.POINTER(RtwSphere)), ("inst_quads", C.POINTER(RtwQuad)),
                ("n_quads", C.c_uint32), ("n_instances", C.c_uint32), ("n_inst_spheres", C.c_uint32), ("n_inst_quads", C.c_uint32)]


class RtwParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("samples", C.c_uint32), ("depth", C.c_uint32),
                ("gamma", C.c_float), ("mint", C.c_float), ("maxt", C.c_float),
                ("integrator", C.c_uint32), ("sampler", C.c_uint32), ("accel", C.c_uint32), ("flags", C.c_uint32),
                ("seed", C.c_uint64),
                ("row_block", C.c_uint32), ("part_index", C.c_uint32), ("part_count", C.c_uint32), ("reserved", C.c_uint32)]


class RtwStats(C.Structure):
    _fields_ = [("camera_rays", C.c_uint64), ("segments", C.c_uint64), ("sphere_tests", C.c_uint64),
                ("node_tests", C.c_uint64), ("nan_pixels", C.c_uint32), ("rows", C.c_uint32),
                ("kernel_ms", C.c_float), ("total_ms", C.c_float),
                ("phase_steps", C.c_uint64 * 6), ("phase_lanes", C.c_uint64 * 6), ("quad_tests", C.c_uint64),
                ("enqueue_ms", C.c_float), ("start_ms", C.c_float)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k.startswith("phase_") else getattr(self, k)) for k, _ in self._fields_}


class RtwPerlin(C.Structure):
    """`PerlinNoise` (Rust/src/texture.rs:61-68) without the never-read ranfloat."""
    _fields_ = [("ranvec", (C.c_float * 3) * 256), ("perm_x", C.c_uint8 * 256), ("perm_y", C.c_uint8 * 256), ("perm_z", C.c_uint8 * 256)]


class RtwTextureNoise(C.Structure):
    """Per texture: `ImageTexture.noise` (index into the tables, -1 = None) and `noise_scale`."""
    _fields_ = [("perlin", C.c_int32), ("scale", C.c_float)]


class RtwBilateral(C.Structure):
    """Arguments of the bilateral post-process: Proximity{size, type}, the input's format, the range term (0 = computed)."""
    _fields_ = [("size", C.c_uint32), ("proximity", C.c_uint32), ("in_format", C.c_uint32), ("avg_gradient", C.c_float)]


class RtwGuidedFilter(C.Structure):
    """Arguments of the guided filter: the bilateral ones, the two sigmas (0 = term off) and same_object (include/rtw.h)."""
    _fields_ = [("base", RtwBilateral), ("sigma_depth", C.c_float), ("sigma_normal", C.c_float), ("same_object", C.c_uint32)]


class RtwAtrous(C.Structure):
    """Arguments of the a-trous filter: levels, the three sigmas (0 = term off), same_object and the albedo floor (include/rtw.h)."""
    _fields_ = [("levels", C.c_uint32), ("sigma_color", C.c_float), ("sigma_depth", C.c_float), ("sigma_normal", C.c_float),
                ("same_object", C.c_uint32), ("albedo_floor", C.c_float)]


class RtwTemporal(C.Structure):
    """Arguments of the temporal accumulation: the two blend floors, the history cap, the depth and normal tests (0 = term off), same_object
    and the pixel offset of both frames' guides (include/rtw.h)."""
    _fields_ = [("alpha", C.c_float), ("alpha_moments", C.c_float), ("max_history", C.c_uint32), ("depth_tol", C.c_float),
                ("normal_cos", C.c_float), ("same_object", C.c_uint32), ("offset", C.c_float * 2)]


class RtwMotionRow(C.Structure):
    """One top-level object's rigid motion for temporal_accumulate(motion=): world points go current -> previous by a (x - from) + to, the
    normals surface_map writes by nrm; moving 0: the object did not move and the rest is not read (include/rtw.h)."""
    _fields_ = [("a", C.c_float * 9), ("from_", C.c_float * 3), ("to", C.c_float * 3), ("nrm", C.c_float * 9), ("moving", C.c_uint32),
                ("pad", C.c_uint32 * 7)]


# RtwMotionRow as a numpy record: what motion_rows and mesh_instance_motion return
MOTION_ROW = np.dtype([("a", np.float32, (3, 3)), ("from", np.float32, 3), ("to", np.float32, 3), ("nrm", np.float32, (3, 3)),
                       ("moving", np.uint32), ("pad", np.uint32, 7)])
assert MOTION_ROW.itemsize == 128 == C.sizeof(RtwMotionRow)


class RtwVarianceEstimate(C.Structure):
    """Arguments of the variance estimate: the history length below which a pixel takes the spatial estimate, its window's radius, the two
    sigmas (0 = term off) and same_object (include/rtw.h)."""
    _fields_ = [("min_history", C.c_uint32), ("radius", C.c_uint32), ("sigma_depth", C.c_float), ("sigma_normal", C.c_float),
                ("same_object", C.c_uint32)]


class RtwSvgf(C.Structure):
    """What the variance-steered a-trous filter takes beside RtwAtrous: sigma_luminance (0 = term off), epsilon and prefilter (include/rtw.h)."""
    _fields_ = [("sigma_luminance", C.c_float), ("epsilon", C.c_float), ("prefilter", C.c_uint32)]


class RtwColourBounds(C.Structure):
    """Arguments of the neighbourhood colour bounds: the window's radius, the box's half-width k in standard deviations, same_object and
    exclude_centre (include/rtw.h)."""
    _fields_ = [("radius", C.c_uint32), ("k", C.c_float), ("same_object", C.c_uint32), ("exclude_centre", C.c_uint32)]


class RtwGuides(C.Structure):
    """One size's guide buffers of the guided upsampling, as surface_map writes them; NULL where not given (include/rtw.h)."""
    _fields_ = [("depth", C.c_void_p), ("normal", C.c_void_p), ("idx", C.c_void_p), ("albedo", C.c_void_p), ("emitted", C.c_void_p)]


class RtwUpsample(C.Structure):
    """Arguments of the guided upsampling: scale, the footprint's radius, the guide sigmas (0 = term off), same_object and the albedo floor
    (include/rtw.h)."""
    _fields_ = [("scale", C.c_uint32), ("radius", C.c_uint32), ("sigma_depth", C.c_float), ("sigma_normal", C.c_float),
                ("same_object", C.c_uint32), ("albedo_floor", C.c_float)]


class RtwMetering(C.Structure):
    """Arguments of rtw_exposure_from_histogram: the shares cut at both ends, the key, the adaptation rate, the level's bounds (include/rtw.h)."""
    _fields_ = [("low_permille", C.c_uint32), ("high_permille", C.c_uint32), ("key", C.c_float), ("rate", C.c_float),
                ("min_level", C.c_float), ("max_level", C.c_float)]


class RtwDisplay(C.Structure):
    """Arguments of the display transform: exposure, tone curve and its white, transfer and its gamma, byte rule, dither, output format
    (include/rtw.h)."""
    _fields_ = [("exposure", C.c_float), ("tone", C.c_uint32), ("white", C.c_float), ("transfer", C.c_uint32), ("gamma", C.c_float),
                ("quantise", C.c_uint32), ("dither", C.c_uint32), ("out_format", C.c_uint32)]


class RtwBloom(C.Structure):
    """Arguments of bloom: levels asked for, the bright pass's threshold and knee, the Karis weight, spread, intensity (include/rtw.h)."""
    _fields_ = [("levels", C.c_uint32), ("threshold", C.c_float), ("knee", C.c_float), ("karis", C.c_uint32), ("spread", C.c_float),
                ("intensity", C.c_float)]


class RtwFilterStats(C.Structure):
    _fields_ = [("avg_gradient", C.c_float), ("spatial", C.c_float), ("gradient_ms", C.c_float), ("table_ms", C.c_float),
                ("filter_ms", C.c_float), ("total_ms", C.c_float), ("taps", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RtwRenderFacts(C.Structure):
    """What a render request needs of its build (include/rtw.h rtw_render_choice): RtwParams' four, and counts (or 0 / 1) of what the scene holds."""
    _fields_ = [(k, C.c_uint32) for k in ("integrator", "sampler", "depth", "flags", "has_textures", "n_quads", "n_instances", "noise",
                                          "n_triangles", "rotations", "placements")]


class RtwTreeFacts(C.Structure):
    """The sphere tree as rtw_bvh_dump describes it, and the scene's sphere count."""
    _fields_ = [(k, C.c_uint32) for k in ("n_nodes", "depth", "n_spheres", "has_f16", "has_planes")]


class RtwRenderChoice(C.Structure):
    _fields_ = [("build", C.c_char * 32)] + [(k, C.c_uint32) for k in ("node_format", "block", "lds_stack_off", "lds_geom_off", "lds_tri_off", "lds_bytes")]


class RtwQueuePlan(C.Structure):
    """The work queue of one band of a render as its launch was handed it (include/rtw.h rtw_ctx_last_queue_plan)."""
    _fields_ = ([(k, C.c_uint32) for k in ("bands", "n_tiles", "tiles_x", "k_base", "k_end", "n_samples", "chunk_len", "n_chunks", "bank_len",
                                           "reg_q1", "reg_q2")]
                + [("reg_len", C.c_uint32 * 3), ("reg_nc", C.c_uint32 * 3)]
                + [(k, C.c_uint32) for k in ("total_work", "sub_shift", "grab_shift", "grab_max", "grid", "block", "has_tile_order",
                                             "row_block", "part_index", "part_count")])

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k in ("reg_len", "reg_nc") else int(getattr(self, k))) for k, _ in self._fields_}


# rtw_ctx_device_math's functions and rtw_ctx_device_sweep's sweeps (include/rtw.h "device math, for tests")
(MATH_SQRT_PLAIN, MATH_SQRT_IEEE, MATH_DIV, MATH_UNIT, MATH_UNIT_BALL, MATH_SPHERE_ROOT, MATH_ATAN2, MATH_ACOS, MATH_SPHERE_UV, MATH_LN, MATH_POW,
 MATH_SINCOS, MATH_EXP) = range(13)
MATH_COLS = {MATH_SQRT_PLAIN: (1, 1), MATH_SQRT_IEEE: (1, 1), MATH_DIV: (2, 1), MATH_UNIT: (3, 3), MATH_UNIT_BALL: (4, 3), MATH_SPHERE_ROOT: (4, 1),
             MATH_ATAN2: (2, 1), MATH_ACOS: (1, 1), MATH_SPHERE_UV: (3, 2), MATH_LN: (1, 1), MATH_POW: (2, 1), MATH_SINCOS: (1, 2), MATH_EXP: (1, 1)}
SWEEP_SQRT, SWEEP_DIV_RANDOM, SWEEP_DIV_MIDPOINT = 0, 1, 2
SWEEP_RECORDS = 16


class RtwSweepRecord(C.Structure):
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32), ("got", C.c_uint32), ("reserved", C.c_uint32)]


class RtwSweepResult(C.Structure):
    """What rtw_ctx_device_sweep reports: counts, the first wrong results (bit patterns) and the kernel's time."""
    _fields_ = [("tested", C.c_uint64), ("wrong", C.c_uint64), ("n_records", C.c_uint32), ("reserved", C.c_uint32),
                ("records", RtwSweepRecord * SWEEP_RECORDS), ("kernel_ms", C.c_float), ("reserved2", C.c_uint32)]

    def failures(self):
        """[(a, b, got)] as hex strings, for a test's message."""
        return [(f"{r.a:#010x}", f"{r.b:#010x}", f"{r.got:#010x}") for r in self.records[:self.n_records]]


_lib = None


def lib() -> C.CDLL:
    """Load librtw_hip.so.  Fails loudly: there is no other implementation to fall back to."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          f"(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    fp = C.POINTER(C.c_float)
    L.rtw_abi_version.restype = C.c_int
    L.rtw_device_count.restype = C.c_int
    L.rtw_strerror.restype = C.c_char_p
    L.rtw_strerror.argtypes = [C.c_int]
    L.rtw_last_hip_error.restype = C.c_int
    L.rtw_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.rtw_ctx_destroy.argtypes = [C.c_void_p]
    L.rtw_ctx_destroy.restype = None
    L.rtw_ctx_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.rtw_ctx_set_scene.argtypes = [C.c_void_p, C.POINTER(RtwScene), C.c_float, C.c_float]
    L.rtw_ctx_render.argtypes = [C.c_void_p, C.POINTER(RtwCamera), C.POINTER(RtwParams), C.c_void_p, C.POINTER(RtwStats)]
    L.rtw_ctx_render_multi.argtypes = [C.c_void_p, C.POINTER(RtwCamera), C.POINTER(RtwParams), C.c_float, C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.POINTER(RtwStats)]
    L.rtw_render.argtypes = [C.POINTER(RtwCamera), C.POINTER(RtwScene), C.POINTER(RtwParams), C.c_void_p, C.POINTER(RtwStats)]
    L.rtw_ctx_set_option.argtypes = [C.c_void_p, C.c_uint32, C.c_double]
    L.rtw_ctx_last_render_build.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.rtw_ctx_last_node_format.argtypes = [C.c_void_p]
    L.rtw_ctx_last_queue_plan.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(RtwQueuePlan)]
    if hasattr(L, "rtw_render_choice"):     # (added within v4: an RTW_HIP_LIB build of the same ABI may predate it)
        L.rtw_render_choice.argtypes = [C.POINTER(RtwRenderFacts), C.POINTER(RtwTreeFacts), C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.POINTER(RtwRenderChoice)]
    L.rtw_mgpu_create.argtypes = [C.POINTER(C.c_int), C.c_uint32, C.POINTER(C.c_void_p)]
    L.rtw_mgpu_destroy.argtypes = [C.c_void_p]
    L.rtw_mgpu_destroy.restype = None
    L.rtw_mgpu_set_scene.argtypes = [C.c_void_p, C.POINTER(RtwScene), C.c_float, C.c_float]
    L.rtw_mgpu_set_option.argtypes = [C.c_void_p, C.c_uint32, C.c_double]
    L.rtw_mgpu_render.argtypes = [C.c_void_p, C.POINTER(RtwCamera), C.POINTER(RtwParams), C.c_void_p, C.POINTER(RtwStats), C.POINTER(RtwStats)]
    L.rtw_render_multi_gpu.argtypes = [C.POINTER(C.c_int), C.c_uint32, C.POINTER(RtwCamera), C.POINTER(RtwScene), C.POINTER(RtwParams),
                                       C.c_void_p, C.POINTER(RtwStats)]
    L.rtw_viewport_new.argtypes = [C.c_uint32, C.c_float, fp, fp, fp, fp, fp, C.POINTER(RtwCamera), C.POINTER(C.c_uint32)]
    L.rtw_viewport_new_from_res.argtypes = [C.c_uint32, C.c_uint32, fp, fp, fp, fp, fp, C.POINTER(RtwCamera), C.POINTER(C.c_uint32)]
    L.rtw_sphere_new.argtypes = [fp, C.c_float, fp, fp, fp, C.POINTER(RtwSphere)]
    L.rtw_sphere_new_with_texture.argtypes = [fp, C.c_float, fp, fp, fp, C.c_int32, C.POINTER(RtwSphere)]
    L.rtw_vec3_rotated.restype = None
    L.rtw_vec3_rotated.argtypes = [fp, fp, fp]
    L.rtw_tile_order.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RtwCamera), C.POINTER(RtwScene), C.POINTER(C.c_uint32), C.c_uint32]
    L.rtw_part_rows.restype = C.c_uint32
    L.rtw_part_rows.argtypes = [C.c_uint32] * 4
    L.rtw_quantize_u8.restype = None
    L.rtw_quantize_u8.argtypes = [fp, C.c_size_t, C.POINTER(C.c_uint8)]
    L.rtw_camera2_new.argtypes = [C.c_float, fp, fp, fp, C.c_float, C.c_float, C.POINTER(RtwCamera)]
    L.rtw_quantize_u8_rust2.restype = None
    L.rtw_quantize_u8_rust2.argtypes = [fp, C.c_size_t, C.POINTER(C.c_uint8)]
    L.rtw_scene_to_json.restype = C.c_size_t
    L.rtw_scene_to_json.argtypes = [C.POINTER(RtwScene), C.c_char_p, C.c_size_t]
    L.rtw_scene_from_json.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(RtwSphere), C.c_uint32, C.POINTER(C.c_uint32),
                                      C.POINTER(RtwTexture), C.c_uint32, C.POINTER(C.c_uint32), fp, C.c_uint32, C.POINTER(C.c_uint32)]
    L.rtw_write_png_f32.argtypes = [C.c_char_p, fp, C.c_uint32, C.c_uint32]
    L.rtw_write_ppm_f32.argtypes = [C.c_char_p, fp, C.c_uint32, C.c_uint32]
    L.rtw_bvh_validate.argtypes = [C.POINTER(RtwScene), C.c_float, C.c_float] + [C.POINTER(C.c_uint32)] * 4
    L.rtw_bvh_dump.argtypes = [C.POINTER(RtwScene), C.c_float, C.c_float, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_int32),
                               C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p]
    L.rtw_bvh_pack_nodes32.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    L.rtw_bvh_query_host.argtypes = [C.POINTER(RtwScene), C.c_float, C.c_float, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                     C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtw_scene_generate.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(RtwSphere), C.c_uint32, C.POINTER(C.c_uint32),
                                     C.POINTER(RtwTexture), C.c_uint32, C.POINTER(C.c_uint32),
                                     fp, C.c_uint32, C.POINTER(C.c_uint32)]
    L.rtw_scene_default_view.argtypes = [C.c_uint32, C.POINTER(RtwCamera), C.POINTER(RtwParams)]
    L.rtw_quad_new.argtypes = [fp, fp, fp, fp, fp, fp, C.POINTER(RtwQuad)]
    L.rtw_box_quads.argtypes = [fp, fp, fp, fp, C.POINTER(RtwQuad)]
    L.rtw_scene_generate_geom.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(RtwSphere), C.POINTER(RtwQuad), C.POINTER(RtwInstance),
                                          C.POINTER(RtwSphere), C.POINTER(RtwQuad), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), fp]
    L.rtw_perlin_new.argtypes = [C.c_uint64, C.POINTER(RtwPerlin)]
    L.rtw_perlin_eval.argtypes = [C.POINTER(RtwPerlin), fp, C.c_uint32, C.c_uint32, fp]
    L.rtw_ctx_perlin_eval.argtypes = [C.c_void_p, C.POINTER(RtwPerlin), fp, C.c_uint32, C.c_uint32, fp]
    L.rtw_ctx_set_texture_noise.argtypes = [C.c_void_p, C.POINTER(RtwPerlin), C.c_uint32, C.POINTER(RtwTextureNoise), C.c_uint32]
    L.rtw_mgpu_set_texture_noise.argtypes = [C.c_void_p, C.POINTER(RtwPerlin), C.c_uint32, C.POINTER(RtwTextureNoise), C.c_uint32]
    L.rtw_bilateral_filter.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(RtwBilateral), C.c_void_p, C.POINTER(RtwFilterStats)]
    L.rtw_ctx_bilateral_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(RtwBilateral), C.c_void_p,
                                           C.POINTER(RtwFilterStats)]
    L.rtw_guided_filter.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtwGuidedFilter), C.c_void_p,
                                    C.POINTER(RtwFilterStats)]
    L.rtw_ctx_guided_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(RtwGuidedFilter), C.c_void_p, C.POINTER(RtwFilterStats)]
    L.rtw_triangle_new.argtypes = [fp, fp, fp, fp, fp, fp, C.c_int32, C.POINTER(RtwTriangle)]
    L.rtw_ctx_set_triangles.argtypes = [C.c_void_p, C.POINTER(RtwTriangle), C.c_uint32]
    L.rtw_mgpu_set_triangles.argtypes = [C.c_void_p, C.POINTER(RtwTriangle), C.c_uint32]
    L.rtw_triangle_bvh_validate.argtypes = [C.POINTER(RtwTriangle), C.c_uint32] + [C.POINTER(C.c_uint32)] * 3
    L.rtw_ctx_refit_triangles.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.rtw_ctx_triangle_bvh_dump.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.rtw_triangle_bvh_dump.argtypes = [C.POINTER(RtwTriangle), C.c_uint32, C.c_void_p, C.c_uint32] + [C.POINTER(C.c_uint32)] * 4
    L.rtw_triangle_bvh_refit.argtypes = [C.POINTER(RtwTriangle), C.c_uint32, fp, C.c_void_p, C.c_uint32] + [C.POINTER(C.c_uint32)] * 2
    L.rtw_triangle_hits.argtypes = [C.POINTER(RtwTriangle), C.c_uint32, fp, C.c_uint32, C.c_float, C.c_float, fp, C.POINTER(C.c_int32)]
    L.rtw_ctx_triangle_hits.argtypes = [C.c_void_p, fp, C.c_uint32, C.c_float, C.c_float, C.c_uint32, fp, C.POINTER(C.c_int32),
                                        C.POINTER(RtwStats)]
    L.rtw_depth_rays.argtypes = [C.POINTER(RtwCamera), C.c_uint32, C.c_uint32, fp]
    L.rtw_ctx_scene_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.POINTER(RtwStats)]
    L.rtw_ctx_scene_surface.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32] + [C.c_void_p] * 6 + [
        C.POINTER(RtwStats)]
    L.rtw_pixel_rays.argtypes = [C.POINTER(RtwCamera), C.c_uint32, C.c_uint32, fp, fp]
    L.rtw_ctx_surface_map.argtypes = [C.c_void_p, C.POINTER(RtwCamera), C.c_uint32, C.c_uint32, C.c_uint32, fp, C.c_float, C.c_float, C.c_float, C.c_uint32,
                                      C.c_uint32] + [C.c_void_p] * 6 + [C.POINTER(RtwStats)]
    L.rtw_ctx_scene_occluded.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_void_p,
                                         C.POINTER(RtwStats)]
    L.rtw_triangle_occluded.argtypes = [C.POINTER(RtwTriangle), C.c_uint32, fp, C.c_uint32, C.c_float, C.c_float, C.c_void_p, C.POINTER(RtwStats)]
    L.rtw_mesh_instance_occluded.argtypes = [C.POINTER(RtwTriangle), C.c_uint32, C.POINTER(RtwMeshInstance), C.c_uint32, fp, C.c_uint32, C.c_float,
                                             C.c_float, C.c_void_p, C.POINTER(RtwStats)]
    L.rtw_ao_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.rtw_ctx_ambient_occlusion.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                            C.c_uint32, C.c_void_p, C.POINTER(RtwStats)]
    L.rtw_ctx_ao_map.argtypes = [C.c_void_p, C.POINTER(RtwCamera), C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32,
                                 C.c_float, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtwStats)]
    L.rtw_ctx_depth_map.argtypes = [C.c_void_p, C.POINTER(RtwCamera), C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtwStats)]
    L.rtw_light_samples.argtypes = [C.POINTER(RtwScene), C.POINTER(RtwLight), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                    C.c_void_p, C.c_void_p]
    L.rtw_light_reduce.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.rtw_ctx_light_count.argtypes = [C.c_void_p]
    L.rtw_ctx_light_count.restype = C.c_uint32
    L.rtw_ctx_direct_light.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                       C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(RtwStats)]
    L.rtw_ctx_direct_light_map.argtypes = [C.c_void_p, C.POINTER(RtwCamera), C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32,
                                           C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(RtwStats)]
    L.rtw_ctx_set_lights.argtypes = [C.c_void_p, C.POINTER(RtwLight), C.c_uint32, C.c_float]
    L.rtw_mgpu_set_lights.argtypes = [C.c_void_p, C.POINTER(RtwLight), C.c_uint32, C.c_float]
    L.rtw_lights_validate.argtypes = [C.POINTER(RtwScene), C.POINTER(RtwLight), C.c_uint32]
    L.rtw_light_mid.argtypes = [C.POINTER(RtwScene), C.POINTER(RtwLight), fp]
    L.rtw_material_pdf.argtypes = [fp, fp, fp, fp, C.c_float, fp, fp, C.c_float]
    L.rtw_material_pdf.restype = C.c_float
    L.rtw_light_term.argtypes = [C.c_uint32, C.c_float, fp, C.c_float, fp, C.c_float, fp, fp]
    L.rtw_mixed_validate.argtypes = [C.POINTER(RtwScene), C.POINTER(RtwParams), C.c_uint32, C.c_uint32]
    L.rtw_mixed_dir.argtypes = [C.c_float, C.c_float, C.c_float, fp, fp]
    L.rtw_mixed_pdf.argtypes = [C.c_float, fp, fp, fp, fp, fp, fp]
    L.rtw_ctx_set_instance_rotations.argtypes = [C.c_void_p, fp, C.c_uint32]
    L.rtw_mgpu_set_instance_rotations.argtypes = [C.c_void_p, fp, C.c_uint32]
    L.rtw_instance_rotations_validate.argtypes = [C.POINTER(RtwScene), fp, C.c_uint32]
    L.rtw_ctx_set_mesh_instances.argtypes = [C.c_void_p, C.POINTER(RtwMeshInstance), C.c_uint32]
    L.rtw_mgpu_set_mesh_instances.argtypes = [C.c_void_p, C.POINTER(RtwMeshInstance), C.c_uint32]
    L.rtw_mesh_instances_validate.argtypes = [C.POINTER(RtwTriangle), C.c_uint32, C.POINTER(RtwMeshInstance), C.c_uint32]
    L.rtw_mesh_instance_hits.argtypes = [C.POINTER(RtwTriangle), C.c_uint32, C.POINTER(RtwMeshInstance), C.c_uint32, fp, C.c_uint32, C.c_float,
                                         C.c_float, fp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), fp]
    L.rtw_ctx_mesh_instance_hits.argtypes = [C.c_void_p, fp, C.c_uint32, C.c_float, C.c_float, C.c_uint32, fp, C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int32), fp, C.POINTER(RtwStats)]
    L.rtw_mesh_top_dump.argtypes = [C.POINTER(RtwTriangle), C.c_uint32, C.POINTER(RtwMeshInstance), C.c_uint32, C.c_void_p, C.c_uint32,
                                    C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.rtw_ctx_move_mesh_instances.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.rtw_ctx_mesh_top_dump.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p]
    L.rtw_mesh_top_refit.argtypes = [C.POINTER(RtwTriangle), C.c_uint32, C.POINTER(RtwMeshInstance), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.rtw_mesh_list_max_default.restype = C.c_uint32
    L.rtw_mesh_list_max_default.argtypes = []
    L.rtw_mesh_instance_hits_tree.argtypes = L.rtw_mesh_instance_hits.argtypes + [C.POINTER(RtwStats)]
    L.rtw_quat_rotate.argtypes = [fp, fp, fp]
    L.rtw_quat_mul.argtypes = [fp, fp, fp]
    L.rtw_quat_from_axis.argtypes = [C.c_float, fp, fp]
    L.rtw_quat_from_euler.argtypes = [fp, fp]
    L.rtw_pow_plain.argtypes = [fp, fp, C.c_size_t, fp]
    L.rtw_sin_plain.argtypes = [fp, C.c_size_t, fp]
    L.rtw_atrous_filter.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5 + [C.POINTER(RtwAtrous), C.c_void_p, C.POINTER(RtwFilterStats)]
    L.rtw_ctx_atrous_filter.argtypes = [C.c_void_p] + L.rtw_atrous_filter.argtypes
    L.rtw_temporal_accumulate.argtypes = ([C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(RtwCamera)] + [C.c_void_p] * 3 + [C.POINTER(RtwCamera)] +
                                          [C.c_void_p] * 6 + [C.POINTER(RtwTemporal)] + [C.c_void_p] * 4 + [C.POINTER(RtwFilterStats)])
    L.rtw_ctx_temporal_accumulate.argtypes = [C.c_void_p] + L.rtw_temporal_accumulate.argtypes
    L.rtw_temporal_accumulate_motion.argtypes = (L.rtw_temporal_accumulate.argtypes[:15] + [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5 +
                                                 [C.POINTER(RtwFilterStats)])
    L.rtw_ctx_temporal_accumulate_motion.argtypes = [C.c_void_p] + L.rtw_temporal_accumulate_motion.argtypes
    L.rtw_mesh_instance_motion.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
    L.rtw_ctx_mesh_instance_motion.argtypes = [C.c_void_p] + L.rtw_mesh_instance_motion.argtypes
    L.rtw_temporal_accumulate_points.argtypes = (L.rtw_temporal_accumulate_motion.argtypes[:18] + [C.c_void_p] * 2 +
                                                 L.rtw_temporal_accumulate_motion.argtypes[18:])
    L.rtw_ctx_temporal_accumulate_points.argtypes = [C.c_void_p] + L.rtw_temporal_accumulate_points.argtypes
    L.rtw_temporal_accumulate_bounded.argtypes = (L.rtw_temporal_accumulate_points.argtypes[:20] + [C.c_void_p] * 2 +
                                                  L.rtw_temporal_accumulate_points.argtypes[20:25] + [C.c_void_p, C.POINTER(RtwFilterStats)])
    L.rtw_ctx_temporal_accumulate_bounded.argtypes = [C.c_void_p] + L.rtw_temporal_accumulate_bounded.argtypes
    L.rtw_colour_bounds.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(RtwColourBounds)] + [C.c_void_p] * 3 + [C.POINTER(RtwFilterStats)]
    L.rtw_ctx_colour_bounds.argtypes = [C.c_void_p] + L.rtw_colour_bounds.argtypes
    L.rtw_upsample_filter.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(RtwGuides), C.c_uint32, C.c_uint32, C.POINTER(RtwGuides),
                                      C.POINTER(RtwUpsample), C.c_void_p, C.c_void_p, C.POINTER(RtwFilterStats)]
    L.rtw_ctx_upsample_filter.argtypes = [C.c_void_p] + L.rtw_upsample_filter.argtypes
    L.rtw_camera_scaled.argtypes = [C.POINTER(RtwCamera), C.c_uint32, C.POINTER(RtwCamera)]
    L.rtw_luminance_histogram.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(RtwFilterStats)]
    L.rtw_ctx_luminance_histogram.argtypes = [C.c_void_p] + L.rtw_luminance_histogram.argtypes
    L.rtw_exposure_from_histogram.argtypes = [C.c_void_p, C.POINTER(RtwMetering), C.c_double, C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_float)]
    L.rtw_display.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(RtwDisplay), C.c_void_p, C.POINTER(RtwFilterStats)]
    L.rtw_ctx_display.argtypes = [C.c_void_p] + L.rtw_display.argtypes
    L.rtw_bloom_levels.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.rtw_bloom_levels.restype = C.c_uint32
    L.rtw_bloom.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(RtwBloom), C.c_void_p, C.c_void_p, C.POINTER(RtwFilterStats)]
    L.rtw_ctx_bloom.argtypes = [C.c_void_p] + L.rtw_bloom.argtypes
    L.rtw_ctx_scene_surface_tri.argtypes = L.rtw_ctx_scene_surface.argtypes[:-1] + [C.c_void_p] * 2 + [C.POINTER(RtwStats)]
    L.rtw_ctx_surface_map_tri.argtypes = L.rtw_ctx_surface_map.argtypes[:-1] + [C.c_void_p] * 2 + [C.POINTER(RtwStats)]
    L.rtw_tri_bary.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtw_mesh_local_rays.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.rtw_deform_motion.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                    C.c_void_p, C.c_void_p]
    L.rtw_ctx_deform_motion.argtypes = [C.c_void_p] + L.rtw_deform_motion.argtypes
    L.rtw_variance_estimate.argtypes = ([C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 3 +
                                        [C.POINTER(RtwVarianceEstimate), C.c_void_p, C.POINTER(RtwFilterStats)])
    L.rtw_ctx_variance_estimate.argtypes = [C.c_void_p] + L.rtw_variance_estimate.argtypes
    L.rtw_svgf_filter.argtypes = ([C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5 +
                                  [C.POINTER(RtwAtrous), C.POINTER(RtwSvgf), C.c_void_p, C.c_void_p, C.POINTER(RtwFilterStats)])
    L.rtw_ctx_svgf_filter.argtypes = [C.c_void_p] + L.rtw_svgf_filter.argtypes
    L.rtw_exp_plain.argtypes = [fp, C.c_size_t, fp]
    L.rtw_cos_plain.argtypes = [fp, C.c_size_t, fp]
    L.rtw_ctx_device_math.argtypes = [C.c_void_p, C.c_uint32, fp, C.c_uint32, C.c_uint32, fp, C.c_uint32]
    L.rtw_ctx_device_sweep.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(RtwSweepResult)]
    L.rtw_rounding_check.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.rtw_sweep_operands.argtypes = [C.c_uint32, C.c_uint64, C.c_size_t, C.c_uint32, C.c_void_p]
    _lib = L
    return L


def _strerror(status: int) -> str:
    try:
        return lib().rtw_strerror(status).decode()
    except Exception:  # library itself missing
        return "?"


def _check(status: int, what: str):
    if status != RTW_OK:
        raise RtwError(status, what)


def _f3(v) -> Optional[C.Array]:
    if v is None:
        return None
    return (C.c_float * 3)(*[float(x) for x in v])


def _fptr(arr):
    return None if arr is None else C.cast(arr, C.POINTER(C.c_float))


def _f1(v):
    return None if v is None else C.pointer(C.c_float(float(v)))


# ---- reference-shaped host objects ---------------------------------------------------------------
class Sphere:
    """`Sphere` of Rust/src/objects/sphere.rs:13-20 (constructors :151-247)."""

    def __init__(self, pod: RtwSphere):
        self.pod = pod

    @staticmethod
    def new(origin, r, col_mod=None, mat=None) -> "Sphere":
        s = RtwSphere()
        _check(lib().rtw_sphere_new(_fptr(_f3(origin)), float(r), _fptr(_f3(col_mod)), _fptr(_f3(mat)), None, C.byref(s)), "rtw_sphere_new")
        return Sphere(s)

    @staticmethod
    def new_moving(origin, r, col_mod, mat, velocity) -> "Sphere":
        s = RtwSphere()
        _check(lib().rtw_sphere_new(_fptr(_f3(origin)), float(r), _fptr(_f3(col_mod)), _fptr(_f3(mat)), _fptr(_f3(velocity)), C.byref(s)), "rtw_sphere_new")
        return Sphere(s)

    @staticmethod
    def new_with_texture(origin, r, col_mod, mat, tex_index: int, velocity=None) -> "Sphere":
        s = RtwSphere()
        _check(lib().rtw_sphere_new_with_texture(_fptr(_f3(origin)), float(r), _fptr(_f3(col_mod)), _fptr(_f3(mat)),
                                                 _fptr(_f3(velocity)), int(tex_index), C.byref(s)), "rtw_sphere_new_with_texture")
        return Sphere(s)

    @staticmethod
    def with_albedo(origin, r, albedo, mat=None, velocity=None) -> "Sphere":
        """Albedo exactly `albedo` (texture = albedo, col_mod = 1): opts out of Sphere::new's c*c quirk."""
        sp = Sphere.new_moving(origin, r, (1.0, 1.0, 1.0), mat, velocity or (0.0, 0.0, 0.0))
        for k in range(3):
            sp.pod.tex_color[k] = float(albedo[k])
        return sp


class Quad:
    """`Quad` of Rust/src/objects/quad.rs:8-20; `new` is :84-110 with ImageTexture::from_color(color)."""

    def __init__(self, pod: RtwQuad):
        self.pod = pod

    @staticmethod
    def new(origin, u, v, mat=None, color=(1.0, 1.0, 1.0), emitted=None, tex_index: int = -1) -> "Quad":
        q = RtwQuad()
        _check(lib().rtw_quad_new(_fptr(_f3(origin)), _fptr(_f3(u)), _fptr(_f3(v)), _fptr(_f3(mat)), _fptr(_f3(emitted)),
                                  _fptr(_f3(color)), C.byref(q)), "rtw_quad_new")
        q.tex = int(tex_index)
        return Quad(q)


class Triangle:
    """Rust2's `Triangle` (Rust2/src/objects/triangle.rs:12-50) with its material and ConstColorTexture / ImageTexture inline."""

    def __init__(self, pod: RtwTriangle):
        self.pod = pod

    @staticmethod
    def new(origin, u, v, mat=None, color=(1.0, 1.0, 1.0), emitted=None, tex_index: int = -1) -> "Triangle":
        t = RtwTriangle()
        _check(lib().rtw_triangle_new(_fptr(_f3(origin)), _fptr(_f3(u)), _fptr(_f3(v)), _fptr(_f3(mat)), _fptr(_f3(emitted)),
                                      _fptr(_f3(color)), int(tex_index), C.byref(t)), "rtw_triangle_new")
        return Triangle(t)

    @staticmethod
    def from_mesh(vertices, faces, mat=None, color=(1.0, 1.0, 1.0), emitted=None, tex_index: int = -1) -> "TriangleArray":
        """An indexed mesh as triangles: face (a, b, c) -> origin = v[a], u = v[b] - v[a], v = v[c] - v[a] (f32).  One material for all."""
        vtx = np.asarray(vertices, np.float32).reshape(-1, 3)
        f = np.asarray(faces, np.int64).reshape(-1, 3)
        if len(f) and (f.min() < 0 or f.max() >= len(vtx)):
            raise ValueError("from_mesh: a face index is outside the vertex array")
        o = vtx[f[:, 0]]
        return TriangleArray(o, vtx[f[:, 1]] - o, vtx[f[:, 2]] - o, mat, color, emitted, tex_index)


class TriangleArray:
    """Many triangles as one ctypes array of RtwTriangle, one material for all.  The derived fields (normal, d, w) are left 0: the library
    recomputes them wherever it reads triangles (rtw.h); Triangle.new fills them."""

    def __init__(self, origin, u, v, mat=None, color=(1.0, 1.0, 1.0), emitted=None, tex_index: int = -1):
        o, uu, vv = (np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (origin, u, v))
        n = len(o)
        self.n = n
        self.arr = (RtwTriangle * max(1, n))()
        rec = np.frombuffer(self.arr, dtype=np.float32, count=max(1, n) * (C.sizeof(RtwTriangle) // 4)).reshape(max(1, n), -1)
        m = np.asarray(mat if mat is not None else SCATTER_M, np.float32)
        rec[:n, 0:3], rec[:n, 3:6], rec[:n, 6:9] = o, uu, vv
        rec[:n, 16:19] = np.asarray(color, np.float32)
        rec[:n, 19:22] = m
        rec[:n, 22:25] = np.asarray(emitted if emitted is not None else (0.0, 0.0, 0.0), np.float32)
        rec[:n, 25].view(np.int32)[:] = int(tex_index)
    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return Triangle(self.arr[i])


def _light_array(lights):
    """(RtwLight array or None, n) of a sequence of (kind, index) pairs / RtwLight."""
    if lights is None or len(lights) == 0:
        return None, 0
    arr = (RtwLight * len(lights))()
    for i, l in enumerate(lights):
        arr[i] = l if isinstance(l, RtwLight) else RtwLight(int(l[0]), int(l[1]))
    return arr, len(lights)


def light_mid(scene: "Scene", light) -> np.ndarray:
    """rtw_light_mid: the mid-point of the light's bounding box, the point its shadow rays aim at ((kind, index) of a top-level sphere / quad)."""
    arr, _ = _light_array([light])
    out = (C.c_float * 3)()
    _check(lib().rtw_light_mid(C.byref(scene.pod), arr, out), "rtw_light_mid")
    return np.array(list(out), np.float32)


def material_pdf(mat, p, n, dir_in, time_in, ray_o, ray_d, ray_time) -> np.float32:
    """rtw_material_pdf: Rust2's material_pdf(h, r) of mat = (metallicness, opacity, ir)."""
    return np.float32(lib().rtw_material_pdf(_f3(mat), _f3(p), _f3(n), _f3(dir_in), float(time_in), _f3(ray_o), _f3(ray_d), float(ray_time)))


def light_term(integrator: int, pdf, e, t, direction, weight, S, count):
    """rtw_light_term: (added, S, count) after one accepted light of the light loop."""
    s = _f3(S)
    c = C.c_float(float(count))
    rc = lib().rtw_light_term(int(integrator), float(pdf), _f3(e), float(t), _f3(direction), float(weight), s, C.byref(c))
    if rc < 0:
        _check(rc, "rtw_light_term")
    return bool(rc), np.array(list(s), np.float32), np.float32(c.value)


def mixed(exp: float):
    """The material triple of Rust2's MixedMaterial::new(exp) under FLAG_MIXED_MATERIAL: (metallicness, opacity, ir) = (0, -1, exp)."""
    return (0.0, -1.0, float(exp))


def render_choice(request: RtwRenderFacts, tree: RtwTreeFacts, lds_geom: int = -1, node_format: int = 0, moving: bool = False,
                  accel: int = ACCEL_BVH) -> dict:
    """rtw_render_choice: the build a render of these facts launches and its dynamic LDS (host only) -- `build` as Renderer.last_render_build()
    writes it, `node_format` as last_node_format(), `block` threads per workgroup, the LDS offsets and size in bytes."""
    out = RtwRenderChoice()
    _check(lib().rtw_render_choice(C.byref(request), C.byref(tree), int(lds_geom), int(node_format), 1 if moving else 0, int(accel), C.byref(out)),
           "rtw_render_choice")
    return {"build": out.build.decode(), **{k: int(getattr(out, k)) for k, _ in RtwRenderChoice._fields_[1:]}}


def mixed_validate(scene: "Scene", params: "RtwParams", n_triangles: int = 0, texture_noise: bool = False) -> int:
    """rtw_mixed_validate: the status a render of `scene` with `params` answers to FLAG_MIXED_MATERIAL (host only)."""
    return int(lib().rtw_mixed_validate(C.byref(scene.pod), C.byref(params), int(n_triangles), 1 if texture_noise else 0))


def mixed_dir(exp, xi_phi, xi_cos, n) -> np.ndarray:
    """rtw_mixed_dir: MixedMaterial::on_hit's direction about the normal n for the two uniform draws (phi's first)."""
    out = (C.c_float * 3)()
    _check(lib().rtw_mixed_dir(float(exp), float(xi_phi), float(xi_cos), _f3(n), out), "rtw_mixed_dir")
    return np.array(list(out), np.float32)


def mixed_pdf(exp, p, n, dir_in, ray_o, ray_d) -> np.float32:
    """rtw_mixed_pdf: MixedMaterial::material_pdf(h, r) for the hit {p, n, incoming direction} and the ray {ray_o, ray_d}."""
    out = C.c_float()
    _check(lib().rtw_mixed_pdf(float(exp), _f3(p), _f3(n), _f3(dir_in), _f3(ray_o), _f3(ray_d), C.byref(out)), "rtw_mixed_pdf")
    return np.float32(out.value)


def _quat_array(quats):
    """(float pointer or None, n, keep-alive array) of a sequence of (w, x, y, z) quaternions."""
    if quats is None or len(quats) == 0:
        return None, 0, None
    arr = np.ascontiguousarray(quats, np.float32)
    assert arr.ndim == 2 and arr.shape[1] == 4, "quaternions are [n][4] = w, x, y, z"
    return arr.ctypes.data_as(C.POINTER(C.c_float)), len(arr), arr


def _f4(q):
    return (C.c_float * 4)(*[float(x) for x in q])


def quat_rotate(q, v) -> np.ndarray:
    """rtw_quat_rotate: Rust2's Quaternion::rotate of v by q = (w, x, y, z) (q need not be normalised)."""
    out = (C.c_float * 3)()
    _check(lib().rtw_quat_rotate(_f4(q), _f3(v), out), "rtw_quat_rotate")
    return np.array(list(out), np.float32)


def quat_mul(a, b) -> np.ndarray:
    """rtw_quat_mul: a.hamilton(b) -- Instance::rotate(rot) is rotation = quat_mul(rotation, rot)."""
    out = (C.c_float * 4)()
    _check(lib().rtw_quat_mul(_f4(a), _f4(b), out), "rtw_quat_mul")
    return np.array(list(out), np.float32)


def quat_from_axis(angle: float, axis) -> np.ndarray:
    """rtw_quat_from_axis: Quaternion::new_from_axis(angle, axis) as (w, x, y, z)."""
    out = (C.c_float * 4)()
    _check(lib().rtw_quat_from_axis(float(angle), _f3(axis), out), "rtw_quat_from_axis")
    return np.array(list(out), np.float32)


def quat_from_euler(euler) -> np.ndarray:
    """rtw_quat_from_euler: Rust2's From<&EulerAngles> for Quaternion, euler = (x, y, z)."""
    out = (C.c_float * 4)()
    _check(lib().rtw_quat_from_euler(_f3(euler), out), "rtw_quat_from_euler")
    return np.array(list(out), np.float32)


def instance_rotations_validate(scene: "Scene", quats) -> int:
    """rtw_instance_rotations_validate: the status rtw_ctx_set_instance_rotations answers for `quats` on `scene` (host only)."""
    ptr, n, _keep = _quat_array(quats)
    return int(lib().rtw_instance_rotations_validate(C.byref(scene.pod), ptr, n))


def _plain1(fn, what, *arrays):
    arrs = np.broadcast_arrays(*[np.asarray(a, np.float32) for a in arrays])
    arrs = [np.ascontiguousarray(a, np.float32) for a in arrs]
    out = np.empty(arrs[0].shape, np.float32)
    fp = C.POINTER(C.c_float)
    _check(fn(*[a.ctypes.data_as(fp) for a in arrs], out.size, out.ctypes.data_as(fp)), what)
    return out


def pow_plain(x, y) -> np.ndarray:
    """rtw_pow_plain over arrays (broadcast): the library's f32 pow for x >= 0, finite y >= 0."""
    return _plain1(lib().rtw_pow_plain, "rtw_pow_plain", x, y)


def exp_plain(x) -> np.ndarray:
    """rtw_exp_plain over an array: the guided filter's f32 exp for x <= 0 (a result below 2^-126 is +0)."""
    return _plain1(lib().rtw_exp_plain, "rtw_exp_plain", x)


def sin_plain(phi) -> np.ndarray:
    """rtw_sin_plain over an array: the library's f32 sin for phi in [0, 2 pi]."""
    return _plain1(lib().rtw_sin_plain, "rtw_sin_plain", phi)


def cos_plain(phi) -> np.ndarray:
    """rtw_cos_plain over an array: the library's f32 cos for phi in [0, 2 pi]."""
    return _plain1(lib().rtw_cos_plain, "rtw_cos_plain", phi)


def _bits(a) -> np.ndarray:
    """f32 values or uint32 bit patterns as a contiguous uint32 array of bit patterns."""
    a = np.asarray(a)
    return np.ascontiguousarray(a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.uint32))


def rounding_check(which: int, a, b, got) -> np.ndarray:
    """rtw_rounding_check (host only): is got[i] the correctly rounded f32 sqrt(a[i]) (SWEEP_SQRT, b ignored) or a[i] / b[i]?  float32 arrays
    or uint32 bit patterns; returns a bool array."""
    a, got = _bits(a), _bits(got)
    b = None if b is None else _bits(b)
    ok = np.empty(a.size, np.uint8)
    _check(lib().rtw_rounding_check(int(which), a.ctypes.data, None if b is None else b.ctypes.data, got.ctypes.data, a.size, ok.ctypes.data),
           "rtw_rounding_check")
    return ok.astype(bool).reshape(a.shape)


def sweep_operands(which: int, first: int, n: int, seed: int):
    """rtw_sweep_operands (host only): the (n, d) pairs a quotient sweep forms for indices first .. first + n - 1, as float32 arrays."""
    out = np.empty((int(n), 2), np.uint32)
    _check(lib().rtw_sweep_operands(int(which), int(first), int(n), int(seed) & 0xFFFFFFFF, out.ctypes.data), "rtw_sweep_operands")
    return out[:, 0].copy().view(np.float32), out[:, 1].copy().view(np.float32)


def _triangle_array(triangles):
    """(ctypes array of RtwTriangle, count) of a TriangleArray or a sequence of Triangle / RtwTriangle."""
    if isinstance(triangles, TriangleArray):
        return triangles.arr, triangles.n
    pods = [t.pod if isinstance(t, Triangle) else t for t in triangles]
    return (RtwTriangle * max(1, len(pods)))(*pods), len(pods)


def _rays(rays):
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    if len(r) == 0:
        raise ValueError("triangle_hits: no rays")
    return r


def triangle_hits(triangles, rays, mint: float, maxt: float):
    """The closest triangle per ray on the host (rtw_triangle_hits, the list walk): rays [n][6] = origin, direction.
    Returns (t [n] float32, +inf on a miss; index [n] int32, -1 on a miss)."""
    arr, n = _triangle_array(triangles)
    r = _rays(rays)
    t = np.empty(len(r), np.float32)
    idx = np.empty(len(r), np.int32)
    _check(lib().rtw_triangle_hits(arr, n, r.ctypes.data_as(C.POINTER(C.c_float)), len(r), float(mint), float(maxt),
                                   t.ctypes.data_as(C.POINTER(C.c_float)), idx.ctypes.data_as(C.POINTER(C.c_int32))), "rtw_triangle_hits")
    return t, idx


def _placement_array(placements):
    """(ctypes array of RtwMeshInstance or None, count) of a sequence of (position, (w, x, y, z)) pairs."""
    if placements is None or len(placements) == 0:
        return None, 0
    arr = (RtwMeshInstance * len(placements))()
    for k, (pos, quat) in enumerate(placements):
        assert len(pos) == 3 and len(quat) == 4, "a placement is (position [3], quaternion [4] = w, x, y, z)"
        arr[k].position[:] = [float(np.float32(x)) for x in pos]
        arr[k].quat[:] = [float(np.float32(x)) for x in quat]
    return arr, len(placements)


def mesh_instances_validate(triangles, placements) -> int:
    """rtw_mesh_instances_validate: the status rtw_ctx_set_mesh_instances answers for `placements` of the mesh `triangles` (host only)."""
    arr, n = _triangle_array(triangles) if triangles is not None and len(triangles) else (None, 0)
    parr, pn = _placement_array(placements)
    return int(lib().rtw_mesh_instances_validate(arr, n, parr, pn))


def _mesh_hit_buffers(n, normals):
    t = np.empty(n, np.float32)
    pl = np.empty(n, np.int32)
    tri = np.empty(n, np.int32)
    nrm = np.empty((n, 3), np.float32) if normals else None
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    return (t, pl, tri, nrm), (t.ctypes.data_as(fp), pl.ctypes.data_as(ip), tri.ctypes.data_as(ip), nrm.ctypes.data_as(fp) if normals else None)


def mesh_instance_hits(triangles, placements, rays, mint: float, maxt: float, normals: bool = True):
    """The closest placement of the mesh per ray on the host (rtw_mesh_instance_hits, the list walk): rays [n][6] = origin, direction.
    Returns (t [n] float32, +inf on a miss; placement [n] int32 and triangle [n] int32, -1 on a miss[; normals [n][3] float32, 0 on a miss])."""
    arr, n = _triangle_array(triangles)
    parr, pn = _placement_array(placements)
    r = _rays(rays)
    out, ptrs = _mesh_hit_buffers(len(r), normals)
    _check(lib().rtw_mesh_instance_hits(arr, n, parr, pn, r.ctypes.data_as(C.POINTER(C.c_float)), len(r), float(mint), float(maxt), *ptrs),
           "rtw_mesh_instance_hits")
    return out if normals else out[:3]


def mesh_instance_hits_tree(triangles, placements, rays, mint: float, maxt: float, normals: bool = True):
    """mesh_instance_hits through the walk the kernels run (rtw_mesh_instance_hits_tree: the top-level tree over the placements, the mesh's tree
    in each placement entered), on the host: (t, placement, triangle, normals or None, RtwStats) -- node_tests counts both trees' visits."""
    arr, n = _triangle_array(triangles)
    parr, pn = _placement_array(placements)
    r = _rays(rays)
    out, ptrs = _mesh_hit_buffers(len(r), normals)
    st = RtwStats()
    _check(lib().rtw_mesh_instance_hits_tree(arr, n, parr, pn, r.ctypes.data_as(C.POINTER(C.c_float)), len(r), float(mint), float(maxt), *ptrs,
                                             C.byref(st)), "rtw_mesh_instance_hits_tree")
    return out + (st,)


def triangle_occluded(triangles, rays, mint: float, maxt: float):
    """Is any triangle in the way of each ray within [mint, maxt]?  On the host (rtw_triangle_occluded: the any-hit walk of the scene
    query's triangle group, through the mesh's tree where the device would take it): (occluded [n] bool, RtwStats).  occluded[i] is
    triangle_hits(...)[1][i] >= 0."""
    arr, n = _triangle_array(triangles)
    r = _rays(rays)
    occ = np.empty(len(r), np.uint8)
    st = RtwStats()
    _check(lib().rtw_triangle_occluded(arr, n, r.ctypes.data_as(C.POINTER(C.c_float)), len(r), float(mint), float(maxt), occ.ctypes.data,
                                       C.byref(st)), "rtw_triangle_occluded")
    return occ.view(np.bool_), st


def mesh_instance_occluded(triangles, placements, rays, mint: float, maxt: float):
    """Is any placement of the mesh in the way of each ray?  On the host (rtw_mesh_instance_occluded: the any-hit walk of the scene query's
    placement group through the top-level tree and the mesh's tree): (occluded [n] bool, RtwStats).  occluded[i] is
    mesh_instance_hits(...)[1][i] >= 0."""
    arr, n = _triangle_array(triangles)
    parr, pn = _placement_array(placements)
    r = _rays(rays)
    occ = np.empty(len(r), np.uint8)
    st = RtwStats()
    _check(lib().rtw_mesh_instance_occluded(arr, n, parr, pn, r.ctypes.data_as(C.POINTER(C.c_float)), len(r), float(mint), float(maxt),
                                            occ.ctypes.data, C.byref(st)), "rtw_mesh_instance_occluded")
    return occ.view(np.bool_), st


TOP_NODE = np.dtype([("lo", np.float32, 3), ("skip", np.uint32), ("hi", np.float32, 3), ("leaf", np.uint32)])


def mesh_top_dump(triangles, placements):
    """rtw_mesh_top_dump: the top-level tree over `placements` of the mesh `triangles` as the device reads it -- (nodes [n_nodes] of TOP_NODE,
    order [n] uint32: the placement indices in leaf order, depth, list_walk)."""
    arr, n = _triangle_array(triangles)
    parr, pn = _placement_array(placements)
    nodes = np.zeros(max(2 * pn, 1), TOP_NODE)                   # (2 n - 1 nodes at the most: SAH may split one placement off per level)
    order = np.zeros(max(pn, 1), np.uint32)
    nn, dp, lw = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(lib().rtw_mesh_top_dump(arr, n, parr, pn, nodes.ctypes.data, len(nodes), C.byref(nn), order.ctypes.data_as(C.POINTER(C.c_uint32)),
                                   C.byref(dp), C.byref(lw)), "rtw_mesh_top_dump")
    return nodes[:nn.value].copy(), order[:pn].copy(), dp.value, lw.value


def _poses(poses, n=None):
    """[n][7] float32 = position, (w, x, y, z) of a list of (position, quat) pairs or an array of that shape."""
    if isinstance(poses, (list, tuple)) and len(poses) and len(poses[0]) == 2:
        poses = [list(pos) + list(quat) for pos, quat in poses]
    a = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
    if n is not None and len(a) != n:
        raise ValueError(f"poses holds {len(a)} placements, the context {n}")
    return a


def mesh_top_refit(triangles, placements, moved=None, ouv=None):
    """rtw_mesh_top_refit: the top-level tree built for `placements` of the mesh `triangles`, refitted on the host to the poses `moved`
    ((position, quat) pairs or [n][7]; None: they stay) with the mesh refitted to ouv (None: it stays) -- the bytes Renderer.mesh_top_dump
    returns after set_mesh_instances(placements) and move_mesh_instances(moved, ouv): (nodes [n_nodes] of TOP_NODE, rows [n][8] float32 =
    normalised quaternion, position, 0; list_walk; n_invalid: the invalid poses of `moved`, whose placements keep their rows)."""
    arr, n = _triangle_array(triangles)
    parr, pn = _placement_array(placements)
    mv = None if moved is None else _poses(moved, pn)
    a = None if ouv is None else _ouv(ouv, n)
    nodes = np.zeros(max(2 * pn, 1), TOP_NODE)
    rows = np.zeros((max(pn, 1), 8), np.float32)
    nn, lw, bad = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(lib().rtw_mesh_top_refit(arr, n, parr, pn, None if mv is None else mv.ctypes.data, None if a is None else a.ctypes.data,
                                    nodes.ctypes.data, len(nodes), C.byref(nn), rows.ctypes.data, C.byref(lw), C.byref(bad)), "rtw_mesh_top_refit")
    return nodes[:nn.value].copy(), rows[:pn].copy(), lw.value, bad.value


def motion_rows(n: int) -> np.ndarray:
    """`n` static motion rows (MOTION_ROW records: moving = 0, a = nrm = I, from = to = 0) for temporal_accumulate(motion=): fill in those
    of the spheres, quads and instances you moved yourself through set_scene (row k belongs to the object surface_map reports as
    motion_first + k) and set their `moving` to 1."""
    rows = np.zeros(int(n), MOTION_ROW)
    rows["a"] = rows["nrm"] = np.eye(3, dtype=np.float32)
    return rows


def mesh_instance_motion(prev_poses, cur_poses):
    """rtw_mesh_instance_motion (host only): the motion rows of mesh placements that went from prev_poses to cur_poses, each a list of
    (position, quat) pairs or an [n][7] array as move_mesh_instances takes them.  Returns (rows [n] of MOTION_ROW, n_invalid): a placement
    whose poses agree byte for byte has moving = 0; one with a pose the placements refuse has NaN in `a` (its pixels get no history) and
    is counted in n_invalid.  Row k is placement k: pass motion_first = Renderer.mesh_instance_first()."""
    pp, cp = _poses(prev_poses), _poses(cur_poses)
    if len(pp) != len(cp):
        raise ValueError(f"mesh_instance_motion: {len(pp)} previous poses, {len(cp)} current ones")
    rows = np.zeros(len(cp), MOTION_ROW)
    bad = C.c_uint32()
    _check(lib().rtw_mesh_instance_motion(pp.ctypes.data, cp.ctypes.data, len(cp), rows.ctypes.data, C.byref(bad)), "rtw_mesh_instance_motion")
    return rows, bad.value


def mesh_local_rays(poses, idx, rays, first: int = 0) -> np.ndarray:
    """rtw_mesh_local_rays (host only): ray i ([n][6]) as placement idx[i] - first of `poses` ((position, quat) pairs or [n_mesh][7]) meets
    it, by the walk's own operations; a ray whose idx names no placement is copied.  The rays tri_bary wants for a placed mesh."""
    pp, r = _poses(poses), _rays(rays)
    ids = np.ascontiguousarray(idx, np.int32).reshape(-1)
    if len(ids) != len(r):
        raise ValueError(f"mesh_local_rays: {len(ids)} ids, {len(r)} rays")
    out = np.empty_like(r)
    _check(lib().rtw_mesh_local_rays(pp.ctypes.data, len(pp), int(first), ids.ctypes.data, r.ctypes.data, len(r), out.ctypes.data), "rtw_mesh_local_rays")
    return out


def tri_bary(ouv, rays, t, tri) -> np.ndarray:
    """rtw_tri_bary (host only): the (alfa, beta) [n][2] float32 that surface_map(bary=True) and scene_surface(bary=True) write, from the
    mesh's ouv rows ([n_tris][9]) alone: for 0 <= tri[i] < n_tris those of ray i ([n][6]) at t[i] inside triangle tri[i], else 0 0.  For a
    placed mesh pass mesh_local_rays(poses, idx, rays, first)."""
    a, r = _ouv(ouv), _rays(rays)
    tt = np.ascontiguousarray(t, np.float32).reshape(-1)
    tr = np.ascontiguousarray(tri, np.int32).reshape(-1)
    if len(tt) != len(r) or len(tr) != len(r):
        raise ValueError(f"tri_bary: {len(r)} rays, {len(tt)} t, {len(tr)} tri")
    out = np.empty((len(r), 2), np.float32)
    _check(lib().rtw_tri_bary(a.ctypes.data, len(a), r.ctypes.data, len(r), tt.ctypes.data, tr.ctypes.data, out.ctypes.data), "rtw_tri_bary")
    return out


def _deform_call(fn, fn_name, head, on_device, tri, bary, prev_ouv, idx, prev_poses, first):
    """rtw_deform_motion / rtw_ctx_deform_motion from the Python arguments of deform_motion."""
    who = "deform_motion"
    shp = tuple(tri.shape)
    n = int(np.prod(shp)) if len(shp) else 1
    keep = []
    ptr = lambda name, a, dtype, shape, writable=False: _atrous_pointer(name, a, dtype, shape, on_device, keep, writable, who)

    def rows(name, a, per):
        if hasattr(a, "data_ptr"):
            if a.numel() % per:
                raise ValueError(f"{who}: {name} must hold [n][{per}] floats")
            return ptr(name, a, np.float32, tuple(a.shape)), a.numel() // per
        b = _poses(a) if per == 7 else _ouv(a)
        keep.append(b)
        return C.c_void_p(b.ctypes.data), len(b)

    op, n_tris = rows("prev_ouv", prev_ouv, 9)
    pp, n_mesh = (None, 0) if prev_poses is None else rows("prev_poses", prev_poses, 7)
    if prev_poses is not None and idx is None:
        raise ValueError(f"{who}: prev_poses needs idx")
    if hasattr(tri, "data_ptr"):
        import torch
        point, normal = (torch.empty(shp + (3,), dtype=torch.float32, device=tri.device) for _ in range(2))
    else:
        point, normal = np.empty(shp + (3,), np.float32), np.empty(shp + (3,), np.float32)
    _check(fn(*head, ptr("tri", tri, np.int32, shp), ptr("bary", bary, np.float32, shp + (2,)), n, op, n_tris,
              ptr("idx", idx if prev_poses is not None else None, np.int32, shp), pp, n_mesh, int(first),
              ptr("prev_point", point, np.float32, shp + (3,), True), ptr("carried_normal", normal, np.float32, shp + (3,), True)), fn_name)
    return point, normal


def deform_motion(tri, bary, prev_ouv, idx=None, prev_poses=None, first: int = 0):
    """rtw_deform_motion (host only), the bytes of Renderer.deform_motion; numpy arrays only.  Arguments and result as there."""
    tri = np.ascontiguousarray(tri, np.int32)
    return _deform_call(lib().rtw_deform_motion, "rtw_deform_motion", (), None, tri, bary, prev_ouv, idx, prev_poses, first)


def depth_rays(cam: RtwCamera, width: int, height: int) -> np.ndarray:
    """The rays of Rust2's Viewport::depth_map for a camera of camera2_new (rtw_depth_rays): [height * width, 6] float32 = origin, unit
    direction, pixel (i, j) at row j * width + i."""
    width, height = int(width), int(height)
    out = np.empty((max(0, width * height), 6), np.float32)
    _check(lib().rtw_depth_rays(C.byref(cam), width, height, out.ctypes.data_as(C.POINTER(C.c_float))), "rtw_depth_rays")
    return out


def pixel_rays(cam: RtwCamera, width: int, height: int, offset=(0.0, 0.0)) -> np.ndarray:
    """The pixel rays of a Viewport camera (rtw_pixel_rays): [height * width, 6] float32 = cam.origin, (pixel00 + delta_u * (i + offset[0])) +
    delta_v * (j + offset[1]), not normalised, pixel (i, j) at row j * width + i.  Offset (0, 0) is SAMPLER_NO_RAND's ray."""
    width, height = int(width), int(height)
    out = np.empty((max(0, width * height), 6), np.float32)
    off = (C.c_float * 2)(float(offset[0]), float(offset[1]))
    _check(lib().rtw_pixel_rays(C.byref(cam), width, height, off, out.ctypes.data_as(C.POINTER(C.c_float))), "rtw_pixel_rays")
    return out


def camera_scaled(cam: RtwCamera, scale: int) -> RtwCamera:
    """The camera whose pixel (I, J) is the scale x scale block of cam's pixels (rtw_camera_scaled): delta_u and delta_v times scale, every
    other field copied.  Render and take the low guides of upsample_filter with it, at ceil(w / scale) x ceil(h / scale)."""
    out = RtwCamera()
    _check(lib().rtw_camera_scaled(C.byref(cam), int(scale), C.byref(out)), "rtw_camera_scaled")
    return out


def _points_normals(what, points, normals):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if len(p) == 0 or len(p) != len(n):
        raise ValueError(f"{what}: points and normals must both hold [n][3] floats, n > 0")
    return p, n


def ao_rays(points, normals, samples: int, seed: int = 0) -> np.ndarray:
    """The rays of ambient occlusion (rtw_ao_rays, host only): [n][samples][6] float32 = origin, direction -- sample k of point i is a
    cosine-weighted direction about normals[i] from points[i], a function of (seed, i, k, point, normal) alone.  A point whose normal is
    exactly (0, 0, 0) is skipped: six zeros for each of its rays.  samples: a power of two in 1 .. 1024."""
    p, n = _points_normals("ao_rays", points, normals)
    out = np.empty((len(p), int(samples), 6), np.float32) if 0 < int(samples) <= 1024 else np.empty((1, 1, 6), np.float32)
    _check(lib().rtw_ao_rays(p.ctypes.data, n.ctypes.data, len(p), int(samples), int(seed) & 0xFFFFFFFF, out.ctypes.data), "rtw_ao_rays")
    return out


def light_samples(scene: "Scene", lights, points, normals, samples: int, seed: int = 0):
    """The segments of direct lighting and their weights (rtw_light_samples, host only): (rays [n][n_lights][samples][6] float32 = origin,
    direction; weights [n][n_lights][samples] float32).  Sample k of point i under light l of `lights` ((kind, index) pairs naming top-level
    spheres / quads of `scene`) runs from points[i] to a point sampled on the light, direction not normalised, a function of
    (seed, i, l, k, point, normal, the light) alone; its weight is the geometric term.  A sample that is not cast (a zero normal, or
    dot(normal, direction) > 0 fails) gets six zeros and the weight 0.  samples: a power of two in 1 .. 1024."""
    p, n = _points_normals("light_samples", points, normals)
    arr, nl = _light_array(lights)
    ok = 0 < int(samples) <= 1024 and 0 < nl <= 16
    rays = np.empty((len(p), nl, int(samples), 6), np.float32) if ok else np.empty((1, 1, 1, 6), np.float32)
    w = np.empty(rays.shape[:3], np.float32)
    _check(lib().rtw_light_samples(C.byref(scene.pod), arr, nl, p.ctypes.data, n.ctypes.data, len(p), int(samples), int(seed) & 0xFFFFFFFF,
                                   rays.ctypes.data, w.ctypes.data), "rtw_light_samples")
    return rays, w


def light_reduce(weights) -> np.ndarray:
    """rtw_light_reduce over the last axis of `weights` ([...][samples] float32): the sum in direct_light's fixed association (lane partials
    over min(samples, 64) lanes, then a halving tree) times 1 / samples.  samples: a power of two in 1 .. 1024."""
    w = np.ascontiguousarray(weights, np.float32)
    if w.ndim == 0 or w.size == 0:
        raise ValueError("light_reduce: weights must hold [...][samples] floats")
    samples = w.shape[-1]
    flat = w.reshape(-1, samples)
    out = np.empty(len(flat), np.float32)
    reduce, src, dst = lib().rtw_light_reduce, flat.ctypes.data, out.ctypes.data
    for j in range(len(flat)):
        _check(reduce(src + 4 * samples * j, samples, dst + 4 * j), "rtw_light_reduce")
    return out.reshape(w.shape[:-1])


def triangle_bvh_validate(triangles):
    """rtw_triangle_bvh_validate: (status, n_nodes, depth, list_walk)."""
    arr, n = _triangle_array(triangles)
    nn, dp, lw = C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = lib().rtw_triangle_bvh_validate(arr, n, C.byref(nn), C.byref(dp), C.byref(lw))
    return rc, nn.value, dp.value, lw.value


def triangle_bvh_dump(triangles):
    """rtw_triangle_bvh_dump: the tree set_triangles builds for `triangles` -- (nodes [n_nodes] of TOP_NODE, order [n] uint32: the triangle
    indices in leaf order, depth, list_walk)."""
    arr, n = _triangle_array(triangles)
    nodes = np.zeros(max(2 * n, 1), TOP_NODE)
    order = np.zeros(max(n, 1), np.uint32)
    nn, dp, lw = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(lib().rtw_triangle_bvh_dump(arr if n else None, n, nodes.ctypes.data, len(nodes), C.byref(nn), order.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       C.byref(dp), C.byref(lw)), "rtw_triangle_bvh_dump")
    return nodes[:nn.value].copy(), order[:n].copy(), dp.value, lw.value


def _ouv(ouv, n=None):
    a = np.ascontiguousarray(ouv, np.float32).reshape(-1, 9)
    if n is not None and len(a) != n:
        raise ValueError(f"ouv holds {len(a)} triangles, the mesh {n}")
    return a


def triangle_bvh_refit(triangles, ouv):
    """rtw_triangle_bvh_refit: the tree of `triangles` refitted on the host to ouv [n][9] = origin, u, v (mesh_ouv) -- the bytes
    Renderer.triangle_bvh_dump returns after Renderer.refit_triangles(ouv): (nodes [n_nodes] of TOP_NODE, list_walk)."""
    arr, n = _triangle_array(triangles)
    a = _ouv(ouv, n)
    nodes = np.zeros(max(2 * n, 1), TOP_NODE)
    nn, lw = C.c_uint32(), C.c_uint32()
    _check(lib().rtw_triangle_bvh_refit(arr if n else None, n, a.ctypes.data_as(C.POINTER(C.c_float)), nodes.ctypes.data, len(nodes), C.byref(nn),
                                        C.byref(lw)), "rtw_triangle_bvh_refit")
    return nodes[:nn.value].copy(), lw.value


def mesh_ouv(vertices, faces) -> np.ndarray:
    """An indexed mesh as Renderer.refit_triangles reads it: [n][9] float32 = origin, u, v per face, Triangle.from_mesh's arithmetic (face
    (a, b, c) -> v[a], v[b] - v[a], v[c] - v[a] in f32).  With torch, on the device:
        torch.cat([v[f[:,0]], v[f[:,1]] - v[f[:,0]], v[f[:,2]] - v[f[:,0]]], 1)"""
    vtx = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) and (f.min() < 0 or f.max() >= len(vtx)):
        raise ValueError("mesh_ouv: a face index is outside the vertex array")
    o = vtx[f[:, 0]]
    return np.ascontiguousarray(np.concatenate([o, vtx[f[:, 1]] - o, vtx[f[:, 2]] - o], 1), np.float32)


def mesh_icosphere(level: int = 2, centre=(0.0, 0.0, 0.0), radius: float = 1.0):
    """A subdivided icosahedron (20 * 4^level faces): (vertices [n][3] float32, faces [m][3] int64), outward winding."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(int(level)):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                cache[key] = len(verts) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    vtx = (np.array(verts) * float(radius) + np.asarray(centre, np.float64)).astype(np.float32)
    return vtx, np.array(f, np.int64)


def mesh_terrain(n_side: int, size: float = 20.0, height: float = 1.0, seed: int = 0, centre=(0.0, 0.0, 0.0)):
    """A height field over an n_side x n_side grid of [-size/2, size/2]^2 in x/z (2 * n_side^2 faces, upward winding): a few smooth
    waves plus seeded noise.  Returns (vertices, faces) as mesh_icosphere."""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-size / 2, size / 2, n_side + 1)
    X, Z = np.meshgrid(xs, xs, indexing="xy")
    Y = height * (0.5 * np.sin(X * 0.7) * np.cos(Z * 0.5) + 0.3 * np.sin(X * 0.23 + Z * 0.31)) + 0.05 * height * rng.standard_normal(X.shape)
    vtx = (np.stack([X, Y, Z], -1).reshape(-1, 3) + np.asarray(centre, np.float64)).astype(np.float32)
    i = np.arange(n_side)
    a = (i[:, None] * (n_side + 1) + i[None, :]).reshape(-1)
    faces = np.concatenate([np.stack([a, a + n_side + 1, a + 1], 1), np.stack([a + 1, a + n_side + 1, a + n_side + 2], 1)])
    return vtx, faces.astype(np.int64)


class Instance:
    """`Instance` of Rust/src/objects/instance.rs:27-38: member spheres and quads, translation, Euler rotation,
    optional constant-density medium (`dist_fn = &const_density; density = d`)."""

    def __init__(self, spheres: Sequence = (), quads: Sequence = ()):
        self.spheres = [s.pod if isinstance(s, Sphere) else s for s in spheres]
        self.quads = [q.pod if isinstance(q, Quad) else q for q in quads]
        self.translation = [0.0, 0.0, 0.0]
        self.rotation = [0.0, 0.0, 0.0]
        self.density, self.medium = 0.0, MEDIUM_SURFACE

    @staticmethod
    def new(spheres, quads) -> "Instance":
        return Instance(spheres, quads)

    @staticmethod
    def new_sphere(spheres) -> "Instance":
        return Instance(spheres, ())

    @staticmethod
    def new_quads(quads) -> "Instance":
        return Instance((), quads)

    @staticmethod
    def new_box(a, b, color, mat) -> "Instance":
        """Instance::new_box (instance.rs:83-176) with ImageTexture::from_color(color)."""
        q = (RtwQuad * 6)()
        _check(lib().rtw_box_quads(_fptr(_f3(a)), _fptr(_f3(b)), _fptr(_f3(mat)), _fptr(_f3(color)), q), "rtw_box_quads")
        return Instance((), [RtwQuad.from_buffer_copy(x) for x in q])

    def translate(self, vec):                      # instance.rs:241-243 (f32 `+=`)
        self.translation = [float(np.float32(a) + np.float32(b)) for a, b in zip(self.translation, vec)]

    def rotate(self, rot):                         # instance.rs:234-236
        self.rotation = [float(np.float32(a) + np.float32(b)) for a, b in zip(self.rotation, rot)]

    def const_density(self, density: float):       # `x.dist_fn = &const_density; x.density = d` (main.rs:355-356)
        self.density, self.medium = float(density), MEDIUM_CONST_DENSITY


class PerlinNoise:
    """`PerlinNoise` (Rust/src/texture.rs:61-194).  `PerlinNoise(seed)` == PerlinNoise::new with the tables drawn from the library's
    PCG32(seed) (the reference draws from the OS: its tables cannot be reproduced); the permutations are the identity, as the reference's
    create_permute leaves them.  noise / turb / value take one point [3] or an array [..., 3] and run on the host (rtw_perlin_eval)."""

    def __init__(self, seed: int = 0):
        self.seed = int(seed)
        self.pod = RtwPerlin()
        _check(lib().rtw_perlin_new(C.c_uint64(self.seed & 0xFFFFFFFFFFFFFFFF), C.byref(self.pod)), "rtw_perlin_new")

    @property
    def ranvec(self) -> np.ndarray:
        return np.ctypeslib.as_array(self.pod.ranvec).reshape(256, 3)

    @property
    def perm(self):
        return tuple(np.ctypeslib.as_array(getattr(self.pod, k)) for k in ("perm_x", "perm_y", "perm_z"))

    def _eval(self, p, depth: int) -> np.ndarray:
        pts = np.ascontiguousarray(p, dtype=np.float32)
        flat = pts.reshape(-1, 3)
        out = np.empty(len(flat), np.float32)
        if len(flat):
            _check(lib().rtw_perlin_eval(C.byref(self.pod), flat.ctypes.data_as(C.POINTER(C.c_float)), len(flat), int(depth),
                                         out.ctypes.data_as(C.POINTER(C.c_float))), "rtw_perlin_eval")
        out = out.reshape(pts.shape[:-1])
        return out[()] if out.ndim == 0 else out

    def noise(self, p):
        """PerlinNoise::noise (texture.rs:154-179)."""
        return self._eval(p, 0)

    def turb(self, p, depth: int):
        """PerlinNoise::turb (texture.rs:181-193); depth 0 is |0| = 0 there, as here."""
        if int(depth) == 0:
            n = np.zeros(np.asarray(p).shape[:-1], np.float32)
            return n[()] if n.ndim == 0 else n
        return self._eval(p, int(depth))

    def value(self, p):
        """PerlinNoise::value (texture.rs:150-152): (1 + noise(p)) * 0.5 in f32."""
        return (np.float32(1.0) + np.asarray(self.noise(p), np.float32)) * np.float32(0.5)


def texture_with_noise(img, scale: float, perlin: Optional[PerlinNoise] = None, seed: int = 0):
    """ImageTexture::new_with_noise(img, width, height, scale) (texture.rs:228-236): (texture array [height][width][3], noise entry) --
    pass the array in Scene(textures=...) and the entry as Scene(noise={its index: entry})."""
    return np.ascontiguousarray(img, dtype=np.float32), (perlin if perlin is not None else PerlinNoise(seed), float(scale))


def texture_from_color_noise(color, scale: float, perlin: Optional[PerlinNoise] = None, seed: int = 0):
    """ImageTexture::from_color_noise(color, scale) (texture.rs:237-245): a 1x1 image of `color` with noise."""
    return texture_with_noise(np.asarray(color, np.float32).reshape(1, 1, 3), scale, perlin, seed)


class Scene:
    """`Scene` (Rust/src/viewport.rs:79-151): spheres (+ image textures), quads, instances, background colour."""

    def __init__(self, spheres: Sequence, textures: Sequence[np.ndarray] = (), background=(0.0, 0.0, 0.0),
                 quads: Sequence = (), instances: Sequence = (), emission_images=None, noise=None, triangles=None):
        """`emission_images` {texture index: index of the texture that is its Rust2 `emmit_img`} (Rust2/src/objects/texture.rs:34-41;
        RTW_INTEGRATOR_RUST2 only).  `noise` {texture index: (PerlinNoise, noise_scale)}: ImageTexture.noise / noise_scale
        (texture.rs:21-27); Renderer / MultiRenderer.set_scene pass it on.  to_json drops it, as the reference's JSON form does."""
        self.noise = dict(noise or {})
        # Rust2 triangles (a TriangleArray or a sequence of Triangle): not part of RtwScene -- Renderer / MultiRenderer.set_scene install them
        # with rtw_ctx_set_triangles when there are some; to_json drops them (the reference's JSON has none)
        self.triangles = None
        self.n_triangles = 0
        if triangles is not None and len(triangles):
            self.triangles, self.n_triangles = _triangle_array(triangles)
        pods = [s.pod if isinstance(s, Sphere) else s for s in spheres]
        self._spheres = (RtwSphere * max(1, len(pods)))(*pods)
        self.n_spheres = len(pods)
        descs, flat, off = [], [], 0
        for img in textures:                      # img: [col(height)][row(width)][3] float32
            img = np.ascontiguousarray(img, dtype=np.float32)
            h, w = img.shape[0], img.shape[1]
            descs.append(RtwTexture(w, h, off, 0))
            flat.append(img.reshape(-1, 3))
            off += w * h
        for t, e in (emission_images or {}).items():
            descs[t].emit_tex = int(e) + 1
        self._textures = (RtwTexture * max(1, len(descs)))(*descs)
        self.n_textures = len(descs)
        self._texels = np.concatenate(flat, axis=0).astype(np.float32) if flat else np.zeros((1, 3), np.float32)
        self.n_texels = off
        self.pod = RtwScene()
        self.pod.spheres = C.cast(self._spheres, C.POINTER(RtwSphere))
        self.pod.textures = C.cast(self._textures, C.POINTER(RtwTexture))
        self.pod.texels = self._texels.ctypes.data_as(C.POINTER(C.c_float))
        self.pod.n_spheres, self.pod.n_textures, self.pod.n_texels = self.n_spheres, self.n_textures, self.n_texels
        for k in range(3):
            self.pod.background[k] = float(background[k])
        self._set_geom([q.pod if isinstance(q, Quad) else q for q in quads], list(instances))

    def _set_geom(self, quads, instances):
        """Flatten quads and instances into the ABI's pools (RtwScene.quads / instances / inst_spheres / inst_quads)."""
        isph, iquad, inst = [], [], []
        for it in instances:
            if isinstance(it, Instance):
                r = RtwInstance(len(isph), len(it.spheres), len(iquad), len(it.quads))
                for k in range(3):
                    r.translation[k], r.rotation[k] = it.translation[k], it.rotation[k]
                r.density, r.medium = it.density, it.medium
                isph += it.spheres
                iquad += it.quads
                inst.append(r)
            else:                                   # (RtwInstance, member spheres, member quads) with absolute ranges
                inst.append(it)
        self._install_geom(quads, inst, isph, iquad)

    def _install_geom(self, quads, inst, isph, iquad):
        self._quads = (RtwQuad * max(1, len(quads)))(*quads)
        self._instances = (RtwInstance * max(1, len(inst)))(*inst)
        self._inst_spheres = (RtwSphere * max(1, len(isph)))(*isph)
        self._inst_quads = (RtwQuad * max(1, len(iquad)))(*iquad)
        self.pod.quads = C.cast(self._quads, C.POINTER(RtwQuad))
        self.pod.instances = C.cast(self._instances, C.POINTER(RtwInstance))
        self.pod.inst_spheres = C.cast(self._inst_spheres, C.POINTER(RtwSphere))
        self.pod.inst_quads = C.cast(self._inst_quads, C.POINTER(RtwQuad))
        self.pod.n_quads, self.pod.n_instances = len(quads), len(inst)
        self.pod.n_inst_spheres, self.pod.n_inst_quads = len(isph), len(iquad)
        self.n_quads, self.n_instances = len(quads), len(inst)

    @staticmethod
    def new_sphere(spheres: Sequence) -> "Scene":
        return Scene(spheres)

    @staticmethod
    def new_quad(quads: Sequence) -> "Scene":
        """Scene::new_quad (viewport.rs:106-121)."""
        return Scene((), quads=quads)

    @staticmethod
    def new(spheres: Sequence, quads: Sequence, instances: Sequence) -> "Scene":
        """Scene::new(spheres, quads, instances) (viewport.rs:122-135); background_color is black."""
        return Scene(spheres, quads=quads, instances=instances)

    @staticmethod
    def generate_geom(which: int, scene_seed: int = 42) -> "Scene":
        """A scene with quads / instances laid out by the host library (SCENE_QUAD_TEST, SCENE_PRESENTATION)."""
        L = lib()
        counts = (C.c_uint32 * 5)()
        bg = (C.c_float * 3)()
        _check(L.rtw_scene_generate_geom(which, scene_seed, None, None, None, None, None, None, counts, bg), "rtw_scene_generate_geom")
        n = [int(x) for x in counts]
        sp, qd, ins = (RtwSphere * max(1, n[0]))(), (RtwQuad * max(1, n[1]))(), (RtwInstance * max(1, n[2]))()
        isp, iqd = (RtwSphere * max(1, n[3]))(), (RtwQuad * max(1, n[4]))()
        caps = (C.c_uint32 * 5)(*n)
        _check(L.rtw_scene_generate_geom(which, scene_seed, sp, qd, ins, isp, iqd, caps, counts, bg), "rtw_scene_generate_geom")
        sc = Scene(list(sp)[:n[0]], background=tuple(bg))
        sc._install_geom(list(qd)[:n[1]], list(ins)[:n[2]], list(isp)[:n[3]], list(iqd)[:n[4]])
        return sc

    def noise_pods(self):
        """The arguments of rtw_ctx_set_texture_noise for `self.noise`: (tables, n_tables, per_texture, n_textures), or None without noise."""
        if not self.noise:
            return None
        tables, index = [], {}
        per = (RtwTextureNoise * max(1, self.n_textures))(*[RtwTextureNoise(-1, 1.0) for _ in range(max(1, self.n_textures))])
        for t, (perlin, scale) in self.noise.items():
            if not 0 <= int(t) < self.n_textures:
                raise RtwError(-1, f"noise for texture {t}: the scene has {self.n_textures} textures")
            if id(perlin) not in index:
                index[id(perlin)] = len(tables)
                tables.append(perlin.pod)
            per[int(t)] = RtwTextureNoise(index[id(perlin)], float(scale))
        tb = (RtwPerlin * len(tables))(*tables)
        return tb, len(tables), per, self.n_textures

    def to_json(self) -> str:
        """`Into<JsonValue> for Scene` (Rust/src/viewport.rs:174-180).  Texture noise is not serialised (texture.rs:268-276)."""
        n = lib().rtw_scene_to_json(C.byref(self.pod), None, 0)
        buf = C.create_string_buffer(n + 1)
        lib().rtw_scene_to_json(C.byref(self.pod), buf, n + 1)
        return buf.value.decode()

    @staticmethod
    def from_json(text: str) -> "Scene":
        """`TryFrom<JsonValue> for Scene` (Rust/src/viewport.rs:181-205); raises RtwError like ParseError."""
        L = lib()
        raw = text.encode()
        ns, nt, nx = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(L.rtw_scene_from_json(raw, len(raw), None, 0, C.byref(ns), None, 0, C.byref(nt), None, 0, C.byref(nx)), "rtw_scene_from_json")
        sp = (RtwSphere * max(1, ns.value))()
        tx = (RtwTexture * max(1, nt.value))()
        tl = np.zeros((max(1, nx.value), 3), np.float32)
        _check(L.rtw_scene_from_json(raw, len(raw), sp, ns.value, C.byref(ns), tx, nt.value, C.byref(nt),
                                     tl.ctypes.data_as(C.POINTER(C.c_float)), nx.value, C.byref(nx)), "rtw_scene_from_json")
        return Scene._from_arrays(sp, ns.value, tx, nt.value, tl, nx.value)

    @staticmethod
    def _from_arrays(sp, ns, tx, nt, tl, nx) -> "Scene":
        sc = Scene(list(sp)[:ns])
        sc._textures, sc.n_textures, sc._texels, sc.n_texels = tx, nt, tl, nx
        sc.pod.textures = C.cast(tx, C.POINTER(RtwTexture))
        sc.pod.texels = tl.ctypes.data_as(C.POINTER(C.c_float))
        sc.pod.n_textures, sc.pod.n_texels = nt, nx
        return sc

    @staticmethod
    def generate(which: int, scene_seed: int = 42) -> "Scene":
        """One of the BASELINE config scenes, laid out by the C++ host library."""
        L = lib()
        ns, nt, nx = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(L.rtw_scene_generate(which, scene_seed, None, 0, C.byref(ns), None, 0, C.byref(nt), None, 0, C.byref(nx)), "rtw_scene_generate")
        sp = (RtwSphere * max(1, ns.value))()
        tx = (RtwTexture * max(1, nt.value))()
        tl = np.zeros((max(1, nx.value), 3), np.float32)
        _check(L.rtw_scene_generate(which, scene_seed, sp, ns.value, C.byref(ns), tx, nt.value, C.byref(nt),
                                    tl.ctypes.data_as(C.POINTER(C.c_float)), nx.value, C.byref(nx)), "rtw_scene_generate")
        return Scene._from_arrays(sp, ns.value, tx, nt.value, tl, nx.value)


class Viewport:
    """`Viewport` of Rust/src/viewport.rs:49-77; `new`/`new_from_res` are :308-428.

    `render(ray_color, scene)` takes the integrator as an enum (a host closure cannot run on the GPU):
    INTEGRATOR_GRADIENT == ray_color_gradient, INTEGRATOR_BG_COLOR == ray_color_bg_color.
    """

    def __init__(self, cam: RtwCamera, width: int, height: int, samples: int, depth: int, gamma: float):
        self.cam, self.width, self.height = cam, width, height
        self.samples, self.depth, self.gamma = samples, depth, gamma
        self.shutter_speed, self.fps, self.frame = 0.0, 30.0, 0
        self.seed = 1
        self.mint, self.maxt = 0.001, 100000.0
        self.flags = 0                       # RtwParams.flags of every render (FLAG_*), passed through unchanged

    @staticmethod
    def new(width, aspect_ratio, samples, depth, gamma, vfov=None, origin=None, direction=None, vup=None, msg=None, lens_radius=None):
        cam, h = RtwCamera(), C.c_uint32()
        _check(lib().rtw_viewport_new(int(width), float(aspect_ratio), _f1(vfov), _fptr(_f3(origin)), _fptr(_f3(direction)),
                                      _fptr(_f3(vup)), _f1(lens_radius), C.byref(cam), C.byref(h)), "rtw_viewport_new")
        return Viewport(cam, int(width), h.value, samples, depth, gamma)

    @staticmethod
    def new_from_res(width, height, samples, depth, gamma, vfov=None, origin=None, direction=None, vup=None, msg=None, lens_radius=None):
        cam, h = RtwCamera(), C.c_uint32()
        _check(lib().rtw_viewport_new_from_res(int(width), int(height), _f1(vfov), _fptr(_f3(origin)), _fptr(_f3(direction)),
                                               _fptr(_f3(vup)), _f1(lens_radius), C.byref(cam), C.byref(h)), "rtw_viewport_new_from_res")
        return Viewport(cam, int(width), h.value, samples, depth, gamma)

    def params(self, integrator=INTEGRATOR_GRADIENT, sampler=SAMPLER_STRATIFIED, accel=ACCEL_BVH) -> RtwParams:
        p = RtwParams()
        p.width, p.height, p.samples, p.depth = self.width, self.height, self.samples, self.depth
        p.gamma, p.mint, p.maxt = self.gamma, self.mint, self.maxt
        p.integrator, p.sampler, p.accel, p.flags, p.seed = integrator, sampler, accel, int(self.flags), self.seed
        p.row_block, p.part_index, p.part_count = 8, 0, 1
        return p

    def camera(self) -> RtwCamera:
        cam = RtwCamera.from_buffer_copy(self.cam)
        cam.time0 = float(np.float32(self.frame) / np.float32(self.fps))    # viewport.rs:279
        cam.shutter = float(self.shutter_speed)
        return cam

    def render(self, ray_color: int, scene: Scene, device: int = 0, accel: int = ACCEL_BVH) -> np.ndarray:
        """Viewport::render (stratified, serial in the reference; viewport.rs:430-478) -> [H][W][3] f32."""
        return self._render(ray_color, SAMPLER_STRATIFIED, scene, device, accel)

    def async_render(self, ray_color: int, scene: Scene, device: int = 0, accel: int = ACCEL_BVH) -> np.ndarray:
        """async_render / render_row (viewport.rs:215-305): exactly `samples` rays, shutter time."""
        return self._render(ray_color, SAMPLER_ROW, scene, device, accel)

    def render_multi(self, ray_color: int, scene: Scene, device: int = 0, accel: int = ACCEL_BVH):
        """render_multi (viewport.rs:249-269): frames start_frame .. start_frame + number_of_frames, each rendered
        with time = frame / fps (the scene and its time-expanded BVH are uploaded once for the whole clip)."""
        start = getattr(self, "start_frame", 0)
        count = getattr(self, "number_of_frames", 1)
        with Renderer(device) as r:
            t0 = float(np.float32(start) / np.float32(self.fps))
            t1 = float(np.float32(start + max(count, 1) - 1) / np.float32(self.fps)) + float(self.shutter_speed)
            r.set_scene(scene, t0, t1)
            p = self.params(ray_color, SAMPLER_ROW, accel)
            video = np.empty((max(count, 0), self.height, self.width, 3), np.float32)
            st = (RtwStats * max(count, 1))()
            cam = self.camera()
            _check(lib().rtw_ctx_render_multi(r._h, C.byref(cam), C.byref(p), float(self.fps), int(start), int(count),
                                              C.c_void_p(video.ctypes.data), st), "rtw_ctx_render_multi")
        self.frame = start + max(count, 1) - 1
        return [video[i] for i in range(count)]

    def render_no_rand(self, ray_color: int, scene: Scene, device: int = 0, accel: int = ACCEL_BVH) -> np.ndarray:
        return self._render(ray_color, SAMPLER_NO_RAND, scene, device, accel)

    def _render(self, ray_color, sampler, scene, device, accel):
        with Renderer(device) as r:
            cam = self.camera()
            r.set_scene(scene, cam.time0, cam.time0 + cam.shutter)
            img, _ = r.render(cam, self.params(ray_color, sampler, accel))
        return img


def raw_stream_handle(hip_stream) -> int:
    """What Renderer.set_stream hands to rtw_ctx_set_stream: the handle as it is; None is 0, the context's own stream."""
    return 0 if hip_stream is None else int(hip_stream)


def torch_stream_handle(stream) -> int:
    """What Renderer.use_torch_stream hands to rtw_ctx_set_stream for a torch.cuda.Stream (anything with a `cuda_stream` handle): the
    handle, or STREAM_LEGACY for torch's default stream, whose handle 0 would select the context's own stream."""
    handle = int(stream.cuda_stream)
    return handle if handle else STREAM_LEGACY


class Renderer:
    """One `rtw_ctx`: one GPU, one stream, device-resident scene + BVH."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().rtw_ctx_create(int(device), C.byref(self._h)), "rtw_ctx_create")
        self._device = int(device)
        self._scene = None
        self._stream = None     # the torch stream of use_torch_stream, kept alive while it is set

    def close(self):
        if self._h:
            lib().rtw_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream: Optional[int]):
        """rtw_ctx_set_stream with a raw HIP stream handle, passed on as it is.  0 / None select the context's OWN stream, which is
        non-blocking and orders with no other stream -- not torch's default stream, whose handle reads 0 as well: that one is
        STREAM_LEGACY, and use_torch_stream picks it."""
        _check(lib().rtw_ctx_set_stream(self._h, C.c_void_p(raw_stream_handle(hip_stream))), "rtw_ctx_set_stream")
        self._stream = None

    def use_torch_stream(self, stream=None):
        """Order every later call of this context on a torch.cuda.Stream: behind what torch has enqueued there, with no synchronise in
        between.  None takes torch.cuda.current_stream of the context's device at the time of this call.  The default stream (handle 0)
        is set as STREAM_LEGACY.  The stream is kept alive by the renderer until another is set."""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(self._device)
        _check(lib().rtw_ctx_set_stream(self._h, C.c_void_p(torch_stream_handle(stream))), "rtw_ctx_set_stream")
        self._stream = stream

    def set_scene(self, scene: Scene, t_begin: float = 0.0, t_end: float = 0.0):
        self._scene = scene     # keep host arrays alive
        _check(lib().rtw_ctx_set_scene(self._h, C.byref(scene.pod), float(t_begin), float(t_end)), "rtw_ctx_set_scene")
        nz = scene.noise_pods()
        if nz is not None:
            _check(lib().rtw_ctx_set_texture_noise(self._h, *nz), "rtw_ctx_set_texture_noise")
        if scene.n_triangles:
            _check(lib().rtw_ctx_set_triangles(self._h, scene.triangles, scene.n_triangles), "rtw_ctx_set_triangles")

    def set_triangles(self, triangles=None):
        """rtw_ctx_set_triangles for the current scene (None: clear them)."""
        if triangles is None or len(triangles) == 0:
            _check(lib().rtw_ctx_set_triangles(self._h, None, 0), "rtw_ctx_set_triangles")
            return
        self._tris = _triangle_array(triangles)
        _check(lib().rtw_ctx_set_triangles(self._h, *self._tris), "rtw_ctx_set_triangles")

    def refit_triangles(self, ouv, n: Optional[int] = None) -> int:
        """rtw_ctx_refit_triangles: move the context's triangles to ouv [n][9] = origin, u, v (mesh_ouv) and refit their tree on the GPU, on
        the context's stream; the topology, the materials and the list order stay, every answer is set_triangles' of the moved mesh.  `ouv`:
        a numpy array (staged); an int device pointer with n= triangles; or anything with data_ptr() -- a torch tensor, float32, contiguous,
        on the context's device, read in place behind its producers on the stream of use_torch_stream, e.g. for vertices v and faces f
            r.refit_triangles(torch.cat([v[f[:,0]], v[f[:,1]] - v[f[:,0]], v[f[:,2]] - v[f[:,0]]], 1))
        Returns list_walk: 1 when a triangle now breaks a condition of the tree and the context walks the list.  Not while placements are set."""
        keep = ouv
        if hasattr(ouv, "data_ptr"):
            if not self._on_device(ouv):
                raise ValueError("refit_triangles: the tensor must be float32, contiguous and on the context's device")
            if ouv.numel() % 9:
                raise ValueError("refit_triangles: the tensor must hold [n][9] floats")
            ptr, cnt = int(ouv.data_ptr()), ouv.numel() // 9
        elif isinstance(ouv, int):
            if n is None:
                raise ValueError("refit_triangles: a device pointer needs n=")
            ptr, cnt = ouv, int(n)
        else:
            keep = _ouv(ouv)
            ptr, cnt = keep.ctypes.data, len(keep)
        if n is not None and int(n) != cnt:
            raise ValueError(f"refit_triangles: ouv holds {cnt} triangles, n = {n}")
        lw = C.c_uint32()
        _check(lib().rtw_ctx_refit_triangles(self._h, C.c_void_p(ptr), cnt, C.byref(lw)), "rtw_ctx_refit_triangles")
        del keep
        return lw.value

    def triangle_bvh_dump(self) -> np.ndarray:
        """rtw_ctx_triangle_bvh_dump: the nodes of the context's triangle tree as the device holds them now ([n_nodes] of TOP_NODE)."""
        nn = C.c_uint32()
        _check(lib().rtw_ctx_triangle_bvh_dump(self._h, None, 0, C.byref(nn)), "rtw_ctx_triangle_bvh_dump")
        nodes = np.zeros(nn.value, TOP_NODE)
        _check(lib().rtw_ctx_triangle_bvh_dump(self._h, nodes.ctypes.data, len(nodes), None), "rtw_ctx_triangle_bvh_dump")
        return nodes

    def set_lights(self, lights=None, biased_weight: float = 100.0):
        """rtw_ctx_set_lights for the current scene: (kind, index) pairs naming top-level spheres / quads (None: clear).  The lights of
        INTEGRATOR_LIGHT_CAST / INTEGRATOR_LIGHT_BIASED; a new scene clears them."""
        arr, n = _light_array(lights)
        _check(lib().rtw_ctx_set_lights(self._h, arr, n, float(biased_weight)), "rtw_ctx_set_lights")

    def set_instance_rotations(self, quats=None):
        """rtw_ctx_set_instance_rotations for the current scene: one (w, x, y, z) per instance (None: clear).  Rust2's quaternion rotation of an
        Instance; renders under INTEGRATOR_RUST2 / _LIGHT_CAST / _LIGHT_BIASED and the scene queries honour it; a new scene clears it."""
        ptr, n, _keep = _quat_array(quats)
        _check(lib().rtw_ctx_set_instance_rotations(self._h, ptr, n), "rtw_ctx_set_instance_rotations")

    def set_mesh_instances(self, placements=None):
        """rtw_ctx_set_mesh_instances: place the context's triangle mesh at every (position, (w, x, y, z)) of `placements` (None: clear).  Rust2's
        Instance of triangles; renders under INTEGRATOR_RUST2 and the scene queries honour it; set_scene and set_triangles clear it."""
        arr, n = _placement_array(placements)
        _check(lib().rtw_ctx_set_mesh_instances(self._h, arr, n), "rtw_ctx_set_mesh_instances")

    def _on_device(self, t, *dtypes) -> bool:
        """Is `t` a torch tensor the C ABI can read or write in place: of one of `dtypes` (none given: float32), contiguous and on the
        context's device?"""
        if not hasattr(t, "data_ptr"):
            return False
        import torch
        return t.dtype in (dtypes or (torch.float32,)) and t.is_contiguous() and t.is_cuda and t.device.index == self._device

    def _device_floats(self, x, per, n, what, name):
        """(pointer, count, keep-alive) of a move's input of `per` floats an entry: a tensor (read in place), an int device pointer with
        its count, or anything numpy reads (staged)."""
        if hasattr(x, "data_ptr"):
            if not self._on_device(x):
                raise ValueError(f"{what}: the tensor must be float32, contiguous and on the context's device")
            if x.numel() % per:
                raise ValueError(f"{what}: the tensor must hold [n][{per}] floats")
            return int(x.data_ptr()), x.numel() // per, x
        if isinstance(x, int):
            if n is None:
                raise ValueError(f"{what}: a device pointer needs {name}=")
            return x, int(n), None
        keep = _poses(x) if per == 7 else _ouv(x)
        return keep.ctypes.data, len(keep), keep

    def move_mesh_instances(self, poses=None, ouv=None, n: Optional[int] = None, n_tris: Optional[int] = None) -> int:
        """rtw_ctx_move_mesh_instances: give the context's placements new poses and / or its mesh new triangles and refit the top-level tree
        (and the mesh's) on the GPU, on the context's stream; both topologies stay, every answer is that of set_triangles + set_mesh_instances
        of the moved mesh and poses.  `poses` (None: they stay): a list of (position, quat) as set_mesh_instances takes it; a numpy [n][7]
        array = position, (w, x, y, z) (staged); an int device pointer with n=; or anything with data_ptr() -- a torch tensor, float32,
        contiguous, on the context's device, read in place behind its producers on the stream of use_torch_stream.  `ouv` (None: the mesh
        stays) as refit_triangles takes it (n_tris= with a device pointer).  Returns list_walk: bit 0 a triangle breaks a condition of the
        mesh's tree, bit 1 a placement or the mesh lies beyond reach and the placements are met in list order.  An invalid pose leaves its
        placement where it was, the others move, and RtwError(E_INVALID) is raised."""
        if poses is None and ouv is None:
            raise ValueError("move_mesh_instances: poses, ouv or both")
        pp, pn, keep_p = (None, 0, None) if poses is None else self._device_floats(poses, 7, n, "move_mesh_instances", "n")
        op, on, keep_o = (None, 0, None) if ouv is None else self._device_floats(ouv, 9, n_tris, "move_mesh_instances", "n_tris")
        if poses is not None and n is not None and int(n) != pn:
            raise ValueError(f"move_mesh_instances: poses holds {pn} placements, n = {n}")
        if ouv is not None and n_tris is not None and int(n_tris) != on:
            raise ValueError(f"move_mesh_instances: ouv holds {on} triangles, n_tris = {n_tris}")
        lw = C.c_uint32()
        _check(lib().rtw_ctx_move_mesh_instances(self._h, C.c_void_p(pp), pn, C.c_void_p(op), on, C.byref(lw)), "rtw_ctx_move_mesh_instances")
        del keep_p, keep_o
        return lw.value

    def mesh_instance_motion(self, prev_poses, cur_poses):
        """rtw_ctx_mesh_instance_motion: mesh_instance_motion's rows on this context's GPU, on its stream, one thread per placement; the same
        bytes.  Each pose argument: a list of (position, quat) pairs or a numpy [n][7] array (staged), or a torch tensor, float32, contiguous,
        on the context's device, read in place behind its producers on the stream of use_torch_stream.  Returns (rows, n_invalid): rows a
        float32 tensor [n][32] on the device when either input is a tensor (hand it to temporal_accumulate(motion=) as it is), else [n] of
        MOTION_ROW."""
        what = "mesh_instance_motion"
        pp, pn, keep_p = self._device_floats(prev_poses, 7, None, what, "n")
        cp, cn, keep_c = self._device_floats(cur_poses, 7, None, what, "n")
        if pn != cn:
            raise ValueError(f"{what}: {pn} previous poses, {cn} current ones")
        like = next((x for x in (cur_poses, prev_poses) if hasattr(x, "data_ptr")), None)
        if like is not None:
            import torch
            rows = torch.empty((cn, 32), dtype=torch.float32, device=like.device)
            rp = int(rows.data_ptr())
        else:
            rows = np.zeros(cn, MOTION_ROW)
            rp = rows.ctypes.data
        bad = C.c_uint32()
        _check(lib().rtw_ctx_mesh_instance_motion(self._h, C.c_void_p(pp), C.c_void_p(cp), cn, C.c_void_p(rp), C.byref(bad)),
               "rtw_ctx_mesh_instance_motion")
        del keep_p, keep_c
        return rows, bad.value

    def deform_motion(self, tri, bary, prev_ouv, idx=None, prev_poses=None, first: int = 0):
        """rtw_ctx_deform_motion: where each pixel's surface point lay a frame ago on a mesh that deformed, on this context's GPU and stream,
        one thread per pixel.  tri [..] int32 and bary [..][2] float32: what surface_map(tri=True, bary=True) wrote for the CURRENT frame;
        prev_ouv [n_tris][9]: the rows refit_triangles took a frame ago (the caller keeps them).  For a placed mesh also idx (surface_map's)
        and prev_poses, the (position, quat) pairs or [n_mesh][7] move_mesh_instances took a frame ago, with first =
        mesh_instance_first().  Every argument is a numpy array (staged) or a contiguous torch tensor on the context's device, read in
        place on the stream of use_torch_stream.  Returns (prev_point, carried_normal), [..][3] float32 each -- tensors when `tri` is one --
        for temporal_accumulate(prev_point=, carried_normal=): NaN in all six where the pixel is not on the mesh (tri outside [0, n_tris),
        idx outside the placements, a refused pose)."""
        if not hasattr(tri, "data_ptr"):
            tri = np.ascontiguousarray(tri, np.int32)
        return _deform_call(lib().rtw_ctx_deform_motion, "rtw_ctx_deform_motion", (self._h,), self._on_device, tri, bary, prev_ouv, idx, prev_poses,
                            first)

    def mesh_instance_first(self) -> int:
        """The top-level index surface_map reports for placement 0 of the context's scene: n_spheres + n_quads + n_instances (0 without a
        scene) -- temporal_accumulate's motion_first for the rows of mesh_instance_motion."""
        sc = self._scene
        return 0 if sc is None else int(sc.pod.n_spheres) + int(sc.pod.n_quads) + int(sc.pod.n_instances)

    def mesh_top_dump(self):
        """rtw_ctx_mesh_top_dump: the context's top-level tree and placement rows as the device holds them now -- (nodes [n_nodes] of TOP_NODE,
        rows [n][8] float32 = normalised quaternion w, x, y, z, position, 0)."""
        nn = C.c_uint32()
        _check(lib().rtw_ctx_mesh_top_dump(self._h, None, 0, C.byref(nn), None), "rtw_ctx_mesh_top_dump")
        nodes = np.zeros(nn.value, TOP_NODE)
        _check(lib().rtw_ctx_mesh_top_dump(self._h, nodes.ctypes.data, len(nodes), None, None), "rtw_ctx_mesh_top_dump")
        rows = np.zeros((int((nodes["leaf"] & 7).sum()), 8), np.float32)         # (every placement sits in exactly one leaf)
        _check(lib().rtw_ctx_mesh_top_dump(self._h, None, 0, None, rows.ctypes.data), "rtw_ctx_mesh_top_dump")
        return nodes, rows

    def mesh_instance_hits(self, rays, mint: float, maxt: float, accel: int = ACCEL_BVH, normals: bool = True):
        """The closest placement of this context's mesh per ray on its GPU (rtw_ctx_mesh_instance_hits): (t, placement, triangle[, normals],
        RtwStats) as mesh_instance_hits."""
        r = _rays(rays)
        out, ptrs = _mesh_hit_buffers(len(r), normals)
        st = RtwStats()
        _check(lib().rtw_ctx_mesh_instance_hits(self._h, r.ctypes.data_as(C.POINTER(C.c_float)), len(r), float(mint), float(maxt), int(accel), *ptrs,
                                                C.byref(st)), "rtw_ctx_mesh_instance_hits")
        return (out if normals else out[:3]) + (st,)

    def triangle_hits(self, rays, mint: float, maxt: float, accel: int = ACCEL_BVH):
        """The closest of this context's triangles per ray on its GPU (rtw_ctx_triangle_hits): (t, index, RtwStats) as triangle_hits."""
        r = _rays(rays)
        t = np.empty(len(r), np.float32)
        idx = np.empty(len(r), np.int32)
        st = RtwStats()
        _check(lib().rtw_ctx_triangle_hits(self._h, r.ctypes.data_as(C.POINTER(C.c_float)), len(r), float(mint), float(maxt), int(accel),
                                           t.ctypes.data_as(C.POINTER(C.c_float)), idx.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st)),
               "rtw_ctx_triangle_hits")
        return t, idx, st

    def scene_hits(self, rays, mint: float, maxt: float, time: float = 0.0, accel: int = ACCEL_BVH, normals: bool = False):
        """The closest hit of each ray ([n][6] = origin, direction; the direction is not normalised) against this context's whole scene
        (rtw_ctx_scene_hits): (t [n] float32, +inf on a miss; top-level index [n] int32 -- spheres, quads, instances, triangles --, -1 on a
        miss[; normals [n][3] float32, 0 on a miss]; RtwStats).  Constant-density instances are skipped."""
        r = _rays(rays)
        t = np.empty(len(r), np.float32)
        idx = np.empty(len(r), np.int32)
        nrm = np.empty((len(r), 3), np.float32) if normals else None
        st = RtwStats()
        _check(lib().rtw_ctx_scene_hits(self._h, r.ctypes.data, len(r), float(time), float(mint), float(maxt), int(accel), t.ctypes.data,
                                        idx.ctypes.data, nrm.ctypes.data if normals else None, C.byref(st)), "rtw_ctx_scene_hits")
        return (t, idx, nrm, st) if normals else (t, idx, st)

    def scene_occluded(self, rays, mint: float, maxt: float, time: float = 0.0, accel: int = ACCEL_BVH, out=None):
        """Is anything of this context's whole scene in the way of each ray ([n][6] = origin, direction; the direction is not normalised)
        within [mint, maxt]?  The any-hit pass (rtw_ctx_scene_occluded): (occluded, RtwStats), occluded[i] exactly scene_hits(...)[1][i] >= 0,
        with the early exit a closest-hit query cannot take.  Constant-density instances are skipped.
        rays: anything numpy reads (staged; occluded is a numpy bool array [n]), or a contiguous float32 torch tensor [n, 6] on the context's
        device: then `out` is a torch.uint8 or torch.bool tensor [n] on the same device (allocated when None), and both are read and written
        in place on the context's stream (use_torch_stream), as refit_triangles reads its tensor."""
        st = RtwStats()
        if hasattr(rays, "data_ptr"):
            import torch
            if not self._on_device(rays):
                raise ValueError("scene_occluded: the rays tensor must be float32, contiguous and on the context's device")
            if rays.numel() == 0 or rays.numel() % 6:
                raise ValueError("scene_occluded: the rays tensor must hold [n][6] floats, n > 0")
            n = rays.numel() // 6
            if out is None:
                out = torch.empty(n, dtype=torch.uint8, device=rays.device)
            if not self._on_device(out, torch.uint8, torch.bool) or out.numel() != n:
                raise ValueError("scene_occluded: out must be a contiguous torch.uint8 or torch.bool tensor [n] on the context's device")
            _check(lib().rtw_ctx_scene_occluded(self._h, C.c_void_p(int(rays.data_ptr())), n, float(time), float(mint), float(maxt), int(accel),
                                                C.c_void_p(int(out.data_ptr())), C.byref(st)), "rtw_ctx_scene_occluded")
            return out, st
        if out is not None:
            raise ValueError("scene_occluded: out= goes with a torch tensor of rays")
        r = _rays(rays)
        occ = np.empty(len(r), np.uint8)
        _check(lib().rtw_ctx_scene_occluded(self._h, r.ctypes.data, len(r), float(time), float(mint), float(maxt), int(accel), occ.ctypes.data,
                                            C.byref(st)), "rtw_ctx_scene_occluded")
        return occ.view(np.bool_), st

    def segments_occluded(self, p, q, lo: float = 1e-3, hi: float = 1.0 - 1e-3, time: float = 0.0, accel: int = ACCEL_BVH):
        """Occlusion between point pairs: is anything between p[i] and q[i] ([n][3] each)?  The rays are (p, q - p) -- one float32 subtraction
        per component, in numpy or in torch as given -- over [lo, hi] in units of the segment, so the defaults leave out both end points'
        own surfaces.  Returns scene_occluded's pair."""
        if hasattr(p, "data_ptr") or hasattr(q, "data_ptr"):
            import torch
            if not (hasattr(p, "data_ptr") and hasattr(q, "data_ptr")) or p.dtype != torch.float32 or q.dtype != torch.float32:
                raise ValueError("segments_occluded: p and q must both be float32 tensors, or both numpy")
            p, q = p.reshape(-1, 3), q.reshape(-1, 3)
            return self.scene_occluded(torch.cat([p, q - p], 1).contiguous(), lo, hi, time, accel)
        p = np.asarray(p, np.float32).reshape(-1, 3)
        q = np.asarray(q, np.float32).reshape(-1, 3)
        return self.scene_occluded(np.concatenate([p, q - p], 1), lo, hi, time, accel)

    def depth_map(self, cam: RtwCamera, width: int, height: int, mint: float, maxt: float, time: float = 0.0, accel: int = ACCEL_BVH,
                  ids: bool = False, normals: bool = False):
        """Rust2's Viewport::depth_map in one launch (rtw_ctx_depth_map), for a camera of camera2_new: (depth [height][width] float32 -- the
        hit's t, maxt * 1.6 on a miss --[, ids [height][width] int32, -1 on a miss][, normals [height][width][3] float32]; RtwStats)."""
        width, height = int(width), int(height)
        depth = np.empty((height, width), np.float32)
        idx = np.empty((height, width), np.int32) if ids else None
        nrm = np.empty((height, width, 3), np.float32) if normals else None
        st = RtwStats()
        _check(lib().rtw_ctx_depth_map(self._h, C.byref(cam), width, height, float(time), float(mint), float(maxt), int(accel), depth.ctypes.data,
                                       idx.ctypes.data if ids else None, nrm.ctypes.data if normals else None, C.byref(st)), "rtw_ctx_depth_map")
        return (depth,) + ((idx,) if ids else ()) + ((nrm,) if normals else ()) + (st,)

    def scene_surface(self, rays, mint: float, maxt: float, integrator: int = INTEGRATOR_BG_COLOR, time: float = 0.0, accel: int = ACCEL_BVH,
                      tri: bool = False, bary: bool = False):
        """scene_hits with the rest of the winner's hit record as the render reads it under `integrator` (rtw_ctx_scene_surface): a dict of
        t [n] float32 (+inf on a miss), idx [n] int32 (-1), normal [n][3], albedo [n][3] (the colour the throughput is multiplied by, textures
        resolved), emitted [n][3], material [n][3] = metallicness, opacity, ir -- all 0 on a miss -- and stats.  tri / bary
        (rtw_ctx_scene_surface_tri): also tri [n] int32, the winning triangle's row of ouv (-1 for every other winner), and bary [n][2], its
        (alfa, beta) (0 0)."""
        r = _rays(rays)
        n = len(r)
        out = dict(t=np.empty(n, np.float32), idx=np.empty(n, np.int32), normal=np.empty((n, 3), np.float32), albedo=np.empty((n, 3), np.float32),
                   emitted=np.empty((n, 3), np.float32), material=np.empty((n, 3), np.float32))
        st = RtwStats()
        six = [out[k].ctypes.data for k in ("t", "idx", "normal", "albedo", "emitted", "material")]
        head = (self._h, r.ctypes.data, n, float(time), float(mint), float(maxt), int(accel), int(integrator))
        if tri or bary:
            if tri:
                out["tri"] = np.empty(n, np.int32)
            if bary:
                out["bary"] = np.empty((n, 2), np.float32)
            _check(lib().rtw_ctx_scene_surface_tri(*head, *six, out["tri"].ctypes.data if tri else None, out["bary"].ctypes.data if bary else None,
                                                   C.byref(st)), "rtw_ctx_scene_surface_tri")
        else:
            _check(lib().rtw_ctx_scene_surface(*head, *six, C.byref(st)), "rtw_ctx_scene_surface")
        out["stats"] = st
        return out

    def surface_map(self, cam: RtwCamera, width: int, height: int, mint: float, maxt: float, integrator: int = INTEGRATOR_BG_COLOR,
                    ray_rule: int = RAYS_PIXEL, offset=(0.5, 0.5), time: float = 0.0, accel: int = ACCEL_BVH, tri: bool = False, bary: bool = False):
        """What a camera sees, in one launch (rtw_ctx_surface_map): a dict of depth [h][w] float32 (maxt * 1.6 on a miss), idx [h][w] int32,
        normal, albedo, emitted, material [h][w][3] and stats.  ray_rule RAYS_PIXEL: a Viewport camera's pixel rays at `offset` inside the
        pixel (pixel_rays); RAYS_DEPTH_MAP: depth_map's rays for a camera of camera2_new.  The guides of Renderer.atrous_filter.  tri / bary
        (rtw_ctx_surface_map_tri): also tri [h][w] int32 and bary [h][w][2] as scene_surface's, the inputs of deform_motion."""
        width, height = int(width), int(height)
        out = dict(depth=np.empty((height, width), np.float32), idx=np.empty((height, width), np.int32))
        for k in ("normal", "albedo", "emitted", "material"):
            out[k] = np.empty((height, width, 3), np.float32)
        off = (C.c_float * 2)(float(offset[0]), float(offset[1]))
        st = RtwStats()
        six = [out[k].ctypes.data for k in ("depth", "idx", "normal", "albedo", "emitted", "material")]
        head = (self._h, C.byref(cam), width, height, int(ray_rule), off, float(time), float(mint), float(maxt), int(accel), int(integrator))
        if tri or bary:
            if tri:
                out["tri"] = np.empty((height, width), np.int32)
            if bary:
                out["bary"] = np.empty((height, width, 2), np.float32)
            _check(lib().rtw_ctx_surface_map_tri(*head, *six, out["tri"].ctypes.data if tri else None, out["bary"].ctypes.data if bary else None,
                                                 C.byref(st)), "rtw_ctx_surface_map_tri")
        else:
            _check(lib().rtw_ctx_surface_map(*head, *six, C.byref(st)), "rtw_ctx_surface_map")
        out["stats"] = st
        return out

    def render_denoised(self, cam: RtwCamera, params: RtwParams, **atrous):
        """Python only: render `params` at gamma 1, take the guides from surface_map at the pixel centres under params' integrator, run
        atrous_filter with albedo and emission (keyword arguments: atrous_filter's), then apply params.gamma as the render does
        (v ** (1 / gamma)).  For Viewport cameras and whole frames (part_count 1).  Returns (frame [h][w][3] float32, RtwStats of the render)."""
        if params.part_count != 1:
            raise ValueError("render_denoised: whole frames only (part_count 1)")
        gamma = float(params.gamma)
        params.gamma = 1.0
        try:
            frame, st = self.render(cam, params)
        finally:
            params.gamma = gamma
        g = self.surface_map(cam, params.width, params.height, params.mint, params.maxt, params.integrator, RAYS_PIXEL, (0.5, 0.5), accel=params.accel)
        out = self.atrous_filter(frame, depth=g["depth"], normal=g["normal"], ids=g["idx"], albedo=g["albedo"], emitted=g["emitted"], **atrous)[0]
        if gamma != 1.0:
            out = np.power(np.maximum(out, np.float32(0.0)), np.float32(1.0 / gamma)).astype(np.float32)
        return out, st

    def ambient_occlusion(self, points, normals, samples: int = 16, radius: float = 1.0, mint: float = 1e-3, seed: int = 0, time: float = 0.0,
                          accel: int = ACCEL_BVH, out=None):
        """Ambient occlusion of points ([n][3]) with normals ([n][3]) against this context's whole scene (rtw_ctx_ambient_occlusion): (ao [n]
        float32, RtwStats), ao[i] the share of `samples` cosine-weighted rays about normals[i] that nothing stops within [mint, radius] --
        exactly (samples - c) / samples, c the count scene_occluded gives for ao_rays(points, normals, samples, seed)[i].  The rays are made and
        walked in one kernel; none is stored.  A point with the normal (0, 0, 0) casts none and answers 1.0.  samples: a power of two in
        1 .. 1024.
        points, normals: anything numpy reads (staged; ao is a numpy array), or contiguous float32 torch tensors on the context's device: then
        `out` is a float32 tensor [n] on the same device (allocated when None), and all three are read and written in place on the
        context's stream (use_torch_stream), as scene_occluded reads its tensor."""
        st = RtwStats()
        args = (int(samples), int(seed) & 0xFFFFFFFF, float(time), float(mint), float(radius), int(accel))
        if hasattr(points, "data_ptr") or hasattr(normals, "data_ptr"):
            import torch
            if not (self._on_device(points) and self._on_device(normals)):
                raise ValueError("ambient_occlusion: points and normals must both be float32 tensors, contiguous and on the context's device")
            if points.numel() == 0 or points.numel() % 3 or normals.numel() != points.numel():
                raise ValueError("ambient_occlusion: points and normals must both hold [n][3] floats, n > 0")
            n = points.numel() // 3
            if out is None:
                out = torch.empty(n, dtype=torch.float32, device=points.device)
            if not self._on_device(out) or out.numel() != n:
                raise ValueError("ambient_occlusion: out must be a contiguous torch.float32 tensor [n] on the context's device")
            _check(lib().rtw_ctx_ambient_occlusion(self._h, C.c_void_p(int(points.data_ptr())), C.c_void_p(int(normals.data_ptr())), n, *args,
                                                   C.c_void_p(int(out.data_ptr())), C.byref(st)), "rtw_ctx_ambient_occlusion")
            return out, st
        if out is not None:
            raise ValueError("ambient_occlusion: out= goes with torch tensors of points and normals")
        p, nrm = _points_normals("ambient_occlusion", points, normals)
        ao = np.empty(len(p), np.float32)
        _check(lib().rtw_ctx_ambient_occlusion(self._h, p.ctypes.data, nrm.ctypes.data, len(p), *args, ao.ctypes.data, C.byref(st)),
               "rtw_ctx_ambient_occlusion")
        return ao, st

    def ao_map(self, cam: RtwCamera, width: int, height: int, mint: float, maxt: float, samples: int = 16, radius: float = 1.0,
               ao_mint: float = 1e-3, seed: int = 0, time: float = 0.0, accel: int = ACCEL_BVH, depth: bool = False, ids: bool = False,
               normals: bool = False):
        """Ambient occlusion of what a camera of camera2_new sees (rtw_ctx_ao_map): depth_map(cam, width, height, mint, maxt) and then
        ambient_occlusion of its hit points, with the normals faced towards the viewer, over [ao_mint, radius], in two launches and with no
        buffer in between on the host: (ao [height][width] float32, 1.0 for a miss pixel[, depth][, ids][, normals] -- depth_map's arrays,
        the normals as it writes them --; RtwStats, the depth pass's counters and rays included)."""
        width, height = int(width), int(height)
        ao = np.empty((height, width), np.float32)
        dep = np.empty((height, width), np.float32) if depth else None
        idx = np.empty((height, width), np.int32) if ids else None
        nrm = np.empty((height, width, 3), np.float32) if normals else None
        st = RtwStats()
        _check(lib().rtw_ctx_ao_map(self._h, C.byref(cam), width, height, float(time), float(mint), float(maxt), int(samples),
                                    int(seed) & 0xFFFFFFFF, float(ao_mint), float(radius), int(accel), ao.ctypes.data,
                                    dep.ctypes.data if depth else None, idx.ctypes.data if ids else None, nrm.ctypes.data if normals else None,
                                    C.byref(st)), "rtw_ctx_ao_map")
        return (ao,) + ((dep,) if depth else ()) + ((idx,) if ids else ()) + ((nrm,) if normals else ()) + (st,)

    def light_count(self) -> int:
        """rtw_ctx_light_count: the lights of the last set_lights (a new scene clears them)."""
        return int(lib().rtw_ctx_light_count(self._h))

    def direct_light(self, points, normals, samples: int = 16, lo: float = 1e-3, hi: float = 1.0 - 1e-3, seed: int = 0, time: float = 0.0,
                     accel: int = ACCEL_BVH, irradiance: bool = True, out_vis=None, out_irr=None):
        """How much of each light of set_lights every point ([n][3], with normals [n][3]) sees (rtw_ctx_direct_light): (vis [n][n_lights]
        float32[, irr [n][n_lights] float32], RtwStats).  Per (point, light) pair, `samples` segments to points sampled on the light's surface
        are made and walked in one kernel over [lo, hi] in units of the segment (segments_occluded's convention); vis is the share that is
        cast (dot(normal, direction) > 0) and reaches the light -- exactly what scene_occluded answers for light_samples' rays --, irr
        light_reduce of their geometric terms: the irradiance for unit radiance, neither the emitted colour nor 1 / pi applied.  A sphere
        light hides the part of its facing hemisphere beyond its own horizon: those samples count as blocked.  samples: a power of two in
        1 .. 1024.
        points, normals: anything numpy reads (staged; numpy arrays come back), or contiguous float32 torch tensors on the context's device:
        then out_vis / out_irr are float32 tensors [n][n_lights] on the same device (allocated when None), and all are read and written in
        place on the context's stream (use_torch_stream), as ambient_occlusion does."""
        st = RtwStats()
        nl = self.light_count()
        args = (int(samples), int(seed) & 0xFFFFFFFF, float(time), float(lo), float(hi), int(accel))
        if hasattr(points, "data_ptr") or hasattr(normals, "data_ptr"):
            import torch
            if not (self._on_device(points) and self._on_device(normals)):
                raise ValueError("direct_light: points and normals must both be float32 tensors, contiguous and on the context's device")
            if points.numel() == 0 or points.numel() % 3 or normals.numel() != points.numel():
                raise ValueError("direct_light: points and normals must both hold [n][3] floats, n > 0")
            n = points.numel() // 3
            if out_vis is None:
                out_vis = torch.empty((n, nl), dtype=torch.float32, device=points.device)
            if irradiance and out_irr is None:
                out_irr = torch.empty((n, nl), dtype=torch.float32, device=points.device)
            for o in (out_vis,) + ((out_irr,) if irradiance else ()):
                if not self._on_device(o) or o.numel() != n * nl:
                    raise ValueError("direct_light: out_vis / out_irr must be contiguous torch.float32 tensors [n][n_lights] on the context's device")
            if not irradiance and out_irr is not None:
                raise ValueError("direct_light: out_irr= goes with irradiance=True")
            _check(lib().rtw_ctx_direct_light(self._h, C.c_void_p(int(points.data_ptr())), C.c_void_p(int(normals.data_ptr())), n, *args,
                                              C.c_void_p(int(out_vis.data_ptr())), C.c_void_p(int(out_irr.data_ptr())) if irradiance else None,
                                              C.byref(st)), "rtw_ctx_direct_light")
            return (out_vis, out_irr, st) if irradiance else (out_vis, st)
        if out_vis is not None or out_irr is not None:
            raise ValueError("direct_light: out_vis= / out_irr= go with torch tensors of points and normals")
        p, nrm = _points_normals("direct_light", points, normals)
        vis = np.empty((len(p), nl), np.float32)
        irr = np.empty((len(p), nl), np.float32) if irradiance else None
        _check(lib().rtw_ctx_direct_light(self._h, p.ctypes.data, nrm.ctypes.data, len(p), *args, vis.ctypes.data,
                                          irr.ctypes.data if irradiance else None, C.byref(st)), "rtw_ctx_direct_light")
        return (vis, irr, st) if irradiance else (vis, st)

    def direct_light_map(self, cam: RtwCamera, width: int, height: int, mint: float, maxt: float, samples: int = 16, lo: float = 1e-3,
                         hi: float = 1.0 - 1e-3, seed: int = 0, time: float = 0.0, accel: int = ACCEL_BVH, irradiance: bool = True,
                         depth: bool = False, ids: bool = False, normals: bool = False):
        """Direct lighting of what a camera of camera2_new sees (rtw_ctx_direct_light_map): depth_map(cam, width, height, mint, maxt) and then
        direct_light of its hit points, with the normals faced towards the viewer, in two launches and with no buffer in between on the
        host: (vis [height][width][n_lights] float32, 0 for a miss pixel[, irr][, depth][, ids][, normals] -- depth_map's arrays, the normals
        as it writes them --; RtwStats, the depth pass's counters and rays included)."""
        width, height = int(width), int(height)
        nl = self.light_count()
        vis = np.empty((height, width, nl), np.float32)
        irr = np.empty((height, width, nl), np.float32) if irradiance else None
        dep = np.empty((height, width), np.float32) if depth else None
        idx = np.empty((height, width), np.int32) if ids else None
        nrm = np.empty((height, width, 3), np.float32) if normals else None
        st = RtwStats()
        _check(lib().rtw_ctx_direct_light_map(self._h, C.byref(cam), width, height, float(time), float(mint), float(maxt), int(samples),
                                              int(seed) & 0xFFFFFFFF, float(lo), float(hi), int(accel), vis.ctypes.data,
                                              irr.ctypes.data if irradiance else None, dep.ctypes.data if depth else None,
                                              idx.ctypes.data if ids else None, nrm.ctypes.data if normals else None, C.byref(st)),
               "rtw_ctx_direct_light_map")
        return (vis,) + ((irr,) if irradiance else ()) + ((dep,) if depth else ()) + ((idx,) if ids else ()) + ((nrm,) if normals else ()) + (st,)

    def set_texture_noise(self, tables=None, n_tables: int = 0, per_texture=None, n_textures: int = 0):
        """rtw_ctx_set_texture_noise as is (no arguments: clear the noise of the current scene)."""
        _check(lib().rtw_ctx_set_texture_noise(self._h, tables, n_tables, per_texture, n_textures), "rtw_ctx_set_texture_noise")

    def perlin_eval(self, perlin: PerlinNoise, p, depth: int = 0) -> np.ndarray:
        """PerlinNoise::noise (depth 0) / turb(p, depth) on this context's GPU (rtw_ctx_perlin_eval)."""
        pts = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)
        out = np.empty(len(pts), np.float32)
        _check(lib().rtw_ctx_perlin_eval(self._h, C.byref(perlin.pod), pts.ctypes.data_as(C.POINTER(C.c_float)), len(pts), int(depth),
                                         out.ctypes.data_as(C.POINTER(C.c_float))), "rtw_ctx_perlin_eval")
        return out

    def device_math(self, fn: int, *columns) -> np.ndarray:
        """rtw_ctx_device_math: one of the hot path's arithmetic sequences (MATH_*) on this context's GPU, element i by thread i (64 consecutive
        elements share a wave).  columns: the function's arguments as arrays (broadcast), or one [n, n_cols] array; returns [n] or
        [n, out_cols] float32."""
        n_cols, out_cols = MATH_COLS[fn]
        if len(columns) == 1 and n_cols > 1:
            arg = np.ascontiguousarray(columns[0], np.float32).reshape(-1, n_cols)
        else:
            arg = np.ascontiguousarray(np.stack(np.broadcast_arrays(*[np.asarray(c, np.float32).ravel() for c in columns]), axis=1), np.float32)
        out = np.empty((len(arg), out_cols), np.float32)
        fp = C.POINTER(C.c_float)
        _check(lib().rtw_ctx_device_math(self._h, int(fn), arg.ctypes.data_as(fp), n_cols, len(arg), out.ctypes.data_as(fp), out_cols),
               "rtw_ctx_device_math")
        return out[:, 0] if out_cols == 1 else out

    def device_sweep(self, which: int, first: int, count: int, seed: int = 0) -> RtwSweepResult:
        """rtw_ctx_device_sweep: sqrt_plain / div_plain over `count` generated arguments from index `first`, each judged exactly on the GPU."""
        res = RtwSweepResult()
        _check(lib().rtw_ctx_device_sweep(self._h, int(which), int(first), int(count), int(seed) & 0xFFFFFFFF, C.byref(res)), "rtw_ctx_device_sweep")
        return res

    def set_option(self, key: int, value: float):
        """Tuning knobs (OPT_*); none of them changes the image."""
        _check(lib().rtw_ctx_set_option(self._h, int(key), float(value)), "rtw_ctx_set_option")

    def last_render_build(self) -> str:
        """Which compiled build of the render kernel this context's last render launched (rtw_ctx_last_render_build), template arguments
        in order: "render_brute<MOVING,SPEC,GEOM>" or "render_bvh<MOVING,NODES,SPEC,GEOM>".  Raises RtwError before the first render."""
        buf = C.create_string_buffer(64)
        _check(lib().rtw_ctx_last_render_build(self._h, buf, len(buf)), "rtw_ctx_last_render_build")
        return buf.value.decode()

    def last_node_format(self) -> int:
        """The format of the tree that build read from LDS (rtw_ctx_last_node_format): NODE_FORMAT_NONE (list walk, or nodes in global
        memory), NODE_FORMAT_F16 or NODE_FORMAT_F32 (OPT_NODE_FORMAT).  Raises RtwError before the first render."""
        rc = lib().rtw_ctx_last_node_format(self._h)
        if rc < 0:
            _check(rc, "rtw_ctx_last_node_format")
        return rc

    def last_queue_plan(self, band: int = 0) -> dict:
        """The work queue the last render handed to its kernel for band `band` (rtw_ctx_last_queue_plan), field by field as RtwQueuePlan;
        reg_len / reg_nc are lists of three.  Raises RtwError before the first render and for band >= last_queue_bands()."""
        q = RtwQueuePlan()
        _check(lib().rtw_ctx_last_queue_plan(self._h, int(band), C.byref(q)), "rtw_ctx_last_queue_plan")
        return q.as_dict()

    def last_queue_bands(self) -> int:
        """How many bands of tile rows the last render was launched in.  Raises RtwError before the first render."""
        return self.last_queue_plan(0)["bands"]

    def bilateral_filter(self, img, size: int, proximity: int = PROXIMITY_SQUARE, avg_gradient: float = 0.0, out=None, shape=None,
                         in_format: Optional[int] = None):
        """Rust2's `bilateral_filter(img, Proximity::new(size, proximity))` on this context's GPU (rtw_ctx_bilateral_filter).
        `img`: a numpy [h][w][3] uint8 array, or float32 (quantised first with Rust2's rule, as quantize_u8_rust2); or an int device
        pointer (e.g. torch_tensor.data_ptr()) with shape=(h, w) and in_format PIXELS_U8 / PIXELS_F32_RUST2.  `out` as in render():
        None -> new numpy uint8 array, numpy array -> host buffer, int -> device pointer of [h][w][3] uint8.  Returns (out, RtwFilterStats)."""
        src, w, h, fmt, _keep = _filter_source("bilateral_filter", img, shape, in_format)
        out, dst = _filter_out(out, h, w)
        st = RtwFilterStats()
        prm = RtwBilateral(int(size), int(proximity), fmt, float(avg_gradient))
        _check(lib().rtw_ctx_bilateral_filter(self._h, src, w, h, C.byref(prm), dst, C.byref(st)), "rtw_ctx_bilateral_filter")
        return out, st

    def guided_filter(self, img, size: int, depth=None, normal=None, ids=None, sigma_depth: float = 0.0, sigma_normal: float = 0.0,
                      same_object: bool = False, proximity: int = PROXIMITY_SQUARE, avg_gradient: float = 0.0, out=None, shape=None,
                      in_format: Optional[int] = None):
        """The bilateral filter guided by depth / normal / object-id buffers on this context's GPU (rtw_ctx_guided_filter, include/rtw.h):
        each tap's weights are multiplied by exp_plain(-(dz^2 / (2 sigma_depth^2) + |dn|^2 / (2 sigma_normal^2))), and by 0 on another
        object with same_object.  `img`, `out`, `shape`, `in_format` as bilateral_filter.  `depth` [h][w] float32, `normal` [h][w][3]
        float32, `ids` [h][w] int32 (what depth_map writes): numpy arrays, or int device pointers; None where the term is off.
        Returns (out, RtwFilterStats)."""
        src, w, h, fmt, _keep = _filter_source("guided_filter", img, shape, in_format)
        guides, _keep_g = _guide_pointers(h, w, depth, normal, ids)
        out, dst = _filter_out(out, h, w)
        st = RtwFilterStats()
        prm = RtwGuidedFilter(RtwBilateral(int(size), int(proximity), fmt, float(avg_gradient)), float(sigma_depth), float(sigma_normal),
                              int(same_object))
        _check(lib().rtw_ctx_guided_filter(self._h, src, w, h, *guides, C.byref(prm), dst, C.byref(st)), "rtw_ctx_guided_filter")
        return out, st

    def atrous_filter(self, frame, depth=None, normal=None, ids=None, albedo=None, emitted=None, levels: int = ATROUS_DEFAULTS["levels"],
                      sigma_color: float = ATROUS_DEFAULTS["sigma_color"], sigma_depth: float = ATROUS_DEFAULTS["sigma_depth"],
                      sigma_normal: float = ATROUS_DEFAULTS["sigma_normal"], same_object: bool = True,
                      albedo_floor: float = ATROUS_DEFAULTS["albedo_floor"], out=None):
        """The edge-avoiding a-trous filter of a linear float32 frame [h][w][3] on this context's GPU (rtw_ctx_atrous_filter, include/rtw.h):
        `levels` passes of a 5 x 5 B-spline kernel stepping by 1, 2, 4 .. pixels, every tap weighed by exp_plain(-(|dc|^2 / (2 sigma_color_i^2)
        + (dz 2^-i)^2 / (2 sigma_depth^2) + |dn|^2 / (2 sigma_normal^2))) and by 0 on another object with same_object.  A sigma of 0 turns
        its term off; a term whose guide is None is off too.  With `albedo` [h][w][3] (and `emitted`) it filters (frame - emitted) / albedo.
        depth [h][w] float32, normal [h][w][3] float32, ids [h][w] int32: what depth_map writes.  Every argument is a numpy array (staged)
        or a contiguous torch tensor on the context's device, read in place on the context's stream (use_torch_stream).  `out`: None -> a
        new array or tensor like `frame`; an array or tensor of the frame's shape, which may be `frame` itself.  Returns (out, RtwFilterStats)."""
        args, h, w, keep = _atrous_arguments(frame, depth, normal, ids, albedo, emitted, self._on_device)
        if out is None:
            if hasattr(frame, "data_ptr"):
                import torch
                out = torch.empty_like(frame)
            else:
                out = np.empty((h, w, 3), np.float32)
        dst = _atrous_pointer("out", out, np.float32, (h, w, 3), self._on_device, keep, writable=True)
        prm = _atrous_params(levels, sigma_color, sigma_depth, sigma_normal, same_object, albedo_floor, depth, normal, ids)
        st = RtwFilterStats()
        _check(lib().rtw_ctx_atrous_filter(self._h, *args, C.byref(prm), dst, C.byref(st)), "rtw_ctx_atrous_filter")
        return out, st

    def temporal_accumulate(self, cur, cam: RtwCamera, depth, normal=None, ids=None, history=None, out_color=None, motion=None,
                            motion_first: int = 0, out_prev_xy=None, prev_point=None, carried_normal=None, hist_lo=None, hist_hi=None,
                            out_clipped=None, **params):
        """Temporal accumulation of a linear float32 frame [h][w][3] on this context's GPU (rtw_ctx_temporal_accumulate, include/rtw.h): the
        previous call's accumulated colour, luminance moments and history length are fetched where each pixel's surface point lay in the
        previous view, each of the four taps accepted or rejected against the guides, and blended with `cur`.  depth [h][w] float32, normal
        [h][w][3] float32, ids [h][w] int32: what surface_map(cam, .., RAYS_PIXEL, offset) writes; a test whose guide is None is off.
        history: None for the first frame, else the dict a previous call returned.  Keyword arguments: alpha, alpha_moments, max_history,
        depth_tol, normal_cos, same_object (TEMPORAL_DEFAULTS) and offset (0.5, 0.5).  Every array is a numpy array (staged) or a contiguous
        torch tensor on the context's device, read in place on the context's stream (use_torch_stream); the results are tensors when `cur` is
        one.  out_color: None -> new; or an array / tensor of the frame's shape, which may be `cur`, never history["color"].
        Returns (history, variance [h][w], RtwFilterStats): history = dict(color, moments, len, depth, normal, idx, cam) holds the results
        and THIS call's guides (not copied: leave them unchanged until the next call has read them) and a copy of cam.  History coverage is
        (history["len"] > 1).mean().
        Moving objects (rtw_ctx_temporal_accumulate_motion): motion -- rows of MOTION_ROW (motion_rows, mesh_instance_motion), a float32
        array [n][32], or a contiguous float32 tensor [n][32] on the context's device -- gives the rigid motion of the objects surface_map
        reports as motion_first .. motion_first + n - 1; their pixels are carried into the previous frame before they are projected.  It
        needs `ids`, whether or not same_object is on.  out_prev_xy: True, or an array / tensor [h][w][2], receives where each pixel lay in
        the previous view (NaN on a first frame) and is returned as history["prev_xy"].  With all three at their defaults the call is
        rtw_ctx_temporal_accumulate.
        Per-pixel motion (rtw_ctx_temporal_accumulate_points): prev_point [h][w][3] float32 -- deform_motion's, or your own -- gives the
        world point each pixel's surface point was a frame ago; a pixel whose prev_point x is not NaN projects that point and takes the four
        taps, whatever its row says, and its normal test reads carried_normal [h][w][3] (None: normal itself).  With both at None the call
        is the one above.
        Bounds on the history (rtw_ctx_temporal_accumulate_bounded): hist_lo and hist_hi [h][w][3] float32, both or neither -- colour_bounds'
        of `cur`, or your own -- clip the reprojected colour of every pixel with a history before it is blended; the moments and the length
        are untouched.  out_clipped: True, or an array / tensor [h][w], receives how far the box moved each pixel's history (summed over the
        channels; 0 without a history) and is returned as history["clipped"].  With all three at None the call is the one above."""
        return _temporal_call(lib().rtw_ctx_temporal_accumulate, "rtw_ctx_temporal_accumulate", (self._h,), self._on_device, cur, cam, depth,
                              normal, ids, history, out_color, params, motion, motion_first, out_prev_xy, lib().rtw_ctx_temporal_accumulate_motion,
                              prev_point, carried_normal, lib().rtw_ctx_temporal_accumulate_points, hist_lo, hist_hi, out_clipped,
                              lib().rtw_ctx_temporal_accumulate_bounded)

    def colour_bounds(self, frame, ids=None, radius: int = BOUNDS_DEFAULTS["radius"], k: float = BOUNDS_DEFAULTS["k"], same_object: bool = False,
                      exclude_centre: bool = False, out_lo=None, out_hi=None, out_clamped=None):
        """mean - k sigma and mean + k sigma, per channel, of a linear float32 frame [h][w][3] over the (2 radius + 1)^2 window around each
        pixel on this context's GPU (rtw_ctx_colour_bounds, include/rtw.h): the box temporal_accumulate(hist_lo=, hist_hi=) clips a
        reprojected colour to, and with exclude_centre (the pixel itself is no tap) and out_clamped the firefly clamp of the frame.  A tap
        outside the frame, one with a channel that is not finite, and with same_object one on another ids [h][w] int32, does not count; a
        pixel without taps gets (-inf, +inf).  Every argument is a numpy array (staged) or a contiguous torch tensor on the context's device,
        read and written in place on the context's stream.  out_lo, out_hi: None -> new arrays or tensors like `frame`.  out_clamped: None
        or False -> not wanted, True -> new, else an array or tensor [h][w][3] of its own.  Returns (lo, hi, clamped or None, RtwFilterStats)."""
        return _bounds_call(lib().rtw_ctx_colour_bounds, "rtw_ctx_colour_bounds", (self._h,), self._on_device, frame, ids, radius, k, same_object,
                            exclude_centre, out_lo, out_hi, out_clamped)

    def upsample_filter(self, frame_lo, size, lo=None, hi=None, scale: int = 2, radius: int = UPSAMPLE_DEFAULTS["radius"],
                        sigma_depth: float = UPSAMPLE_DEFAULTS["sigma_depth"], sigma_normal: float = UPSAMPLE_DEFAULTS["sigma_normal"],
                        same_object: bool = UPSAMPLE_DEFAULTS["same_object"], albedo_floor: float = UPSAMPLE_DEFAULTS["albedo_floor"], out=None,
                        out_wsum=False):
        """A linear float32 frame [h_lo][w_lo][3] reconstructed at size = (w, h) on this context's GPU (rtw_ctx_upsample_filter,
        include/rtw.h), with w_lo = ceil(w / scale) and h_lo = ceil(h / scale): joint bilateral upsampling of (frame - emitted) / albedo.
        Every output pixel takes the 2 x 2 (radius 1, bilinear) or 4 x 4 (radius 2, a tent) low pixels about its centre, each weighed by
        exp_plain(-((dz / scale)^2 / (2 sigma_depth^2) + |dn|^2 / (2 sigma_normal^2))) between the LOW guide of the tap and the OUTPUT-size
        guide of the pixel, and by 0 on another object with same_object; the result is multiplied by the output-size albedo and the
        output-size emission added.  A pixel no tap reaches takes its covering low pixel.  lo, hi: dicts as surface_map returns them, at
        the low size (taken with camera_scaled(cam, scale)) and at the output size; only the keys a term needs are read -- depth with
        sigma_depth > 0, normal with sigma_normal > 0, idx with same_object -- and albedo and emitted where present.  Every array is a numpy
        array (staged) or a contiguous torch tensor on the context's device, read and written in place on the context's stream.  out: None
        -> a new array or tensor like frame_lo.  out_wsum: None or False -> not wanted, True -> new, else an array or tensor [h][w]; it
        receives every pixel's weight sum, 0 exactly where the fallback was taken.  Returns (out, wsum or None, RtwFilterStats)."""
        return _upsample_call(lib().rtw_ctx_upsample_filter, "rtw_ctx_upsample_filter", (self._h,), self._on_device, frame_lo, size, lo, hi, scale,
                              radius, sigma_depth, sigma_normal, same_object, albedo_floor, out, out_wsum)

    def render_upsampled(self, cam: RtwCamera, params: RtwParams, scale: int, atrous=None, **upsample):
        """Python only: render at ceil(width / scale) x ceil(height / scale) with camera_scaled(cam, scale) at gamma 1, take the low guides
        there at the pixel centres, optionally run atrous_filter at the low size with albedo and emission (atrous: a dict of its keyword
        arguments, None = no filter), take the guides at params' size with `cam`, run upsample_filter (keyword arguments: its own), then
        apply params.gamma as render_denoised does.  For Viewport cameras and whole frames (part_count 1).  Returns (frame [h][w][3]
        float32, RtwStats of the render)."""
        if params.part_count != 1:
            raise ValueError("render_upsampled: whole frames only (part_count 1)")
        lcam, lp = _scaled_view(cam, params, int(scale))
        lp.gamma = 1.0
        frame, st = self.render(lcam, lp)
        surf = lambda c, p: self.surface_map(c, p.width, p.height, p.mint, p.maxt, p.integrator, RAYS_PIXEL, (0.5, 0.5), accel=p.accel)
        g = surf(lcam, lp)
        if atrous is not None:
            frame = self.atrous_filter(frame, depth=g["depth"], normal=g["normal"], ids=g["idx"], albedo=g["albedo"], emitted=g["emitted"], **atrous)[0]
        out = self.upsample_filter(frame, (params.width, params.height), lo=g, hi=surf(cam, params), scale=scale, **upsample)[0]
        gamma = float(params.gamma)
        if gamma != 1.0:
            out = np.power(np.maximum(out, np.float32(0.0)), np.float32(1.0 / gamma)).astype(np.float32)
        return out, st

    def luminance_histogram(self, frame, out_hist=None, out_counts=None):
        """The luminance histogram of a linear float32 frame [h][w][3] on this context's GPU (rtw_ctx_luminance_histogram, include/rtw.h):
        eight bins a stop over 2^-16 .. 2^16 of Y = 0.2126 r + 0.7152 g + 0.0722 b, the black (Y <= 0) and the non-finite pixels counted
        apart.  frame: a numpy array (staged) or a contiguous torch tensor on the context's device, read in place on the context's
        stream.  out_hist (uint32 [256]) and out_counts (uint32 [2] = black, non_finite): None -> new arrays, or tensors like `frame` when
        it is one (torch has no uint32: int32 tensors, whose bits are the counts); a numpy array or such an int32 tensor otherwise.
        Returns (hist, counts, RtwFilterStats)."""
        return _histogram_call(lib().rtw_ctx_luminance_histogram, "rtw_ctx_luminance_histogram", (self._h,), self._on_device, frame, out_hist,
                               out_counts)

    def display(self, frame, out=None, **params):
        """The display transform of a linear float32 frame [h][w][3] on this context's GPU (rtw_ctx_display, include/rtw.h): exposure, tone
        curve, clamp, transfer function, then bytes or float32.  params: DISPLAY_DEFAULTS' keys.  frame: a numpy array (staged) or a
        contiguous torch tensor on the context's device, read in place on the context's stream.  out: None -> a new array, or a tensor when
        `frame` is one; else a C-contiguous numpy array or a contiguous tensor on the device of [h][w][3] uint8 (DISPLAY_RGB8), [h][w][4]
        uint8 (DISPLAY_RGBA8) or [h][w][3] float32 (DISPLAY_F32), which must not overlap `frame`.  Returns (out, RtwFilterStats)."""
        return _display_call(lib().rtw_ctx_display, "rtw_ctx_display", (self._h,), self._on_device, frame, out, params)

    def bloom(self, frame, out=None, layer=False, **params):
        """Bloom of a linear float32 frame [h][w][3] on this context's GPU (rtw_ctx_bloom, include/rtw.h): a bright pass (threshold, knee,
        the Karis weight), a pyramid of `levels` 13-tap down steps and tent up steps (spread), and out = frame + intensity * layer.
        params: BLOOM_DEFAULTS' keys.  frame: a numpy array (staged) or a contiguous torch tensor on the context's device, read in place
        on the context's stream.  out: None -> a new array, or a tensor when `frame` is one; else a C-contiguous numpy array or a
        contiguous tensor on the device of [h][w][3] float32, which may be `frame` itself and must not overlap it otherwise.  layer:
        False -> no layer; True -> a new array or tensor like `frame`; else such a buffer, overlapping neither.
        Returns (out, layer or None, RtwFilterStats)."""
        return _bloom_call(lib().rtw_ctx_bloom, "rtw_ctx_bloom", (self._h,), self._on_device, frame, out, layer, params)

    def variance_estimate(self, moments, length, depth=None, normal=None, ids=None, min_history: int = SVGF_DEFAULTS["min_history"],
                          radius: int = SVGF_DEFAULTS["radius"], sigma_depth: float = SVGF_DEFAULTS["sigma_depth"],
                          sigma_normal: float = SVGF_DEFAULTS["sigma_normal"], same_object: bool = True, out=None):
        """A luminance variance [h][w] for every pixel of an accumulated frame on this context's GPU (rtw_ctx_variance_estimate,
        include/rtw.h): where length >= min_history the variance over time of the two moments, elsewhere the variance of the moments'
        weighted mean over a (2 radius + 1)^2 window of pixels on the same surface, times min_history / length.  moments [h][w][2] and
        length [h][w] float32: temporal_accumulate's history["moments"] and history["len"]; the guides and their terms as atrous_filter's.
        min_history 1 turns the spatial estimate off.  Every argument is a numpy array (staged) or a contiguous torch tensor on the
        context's device, read in place on the context's stream; `out`: None -> a new array or tensor like `moments`.  Returns
        (variance, RtwFilterStats)."""
        return _variance_call(lib().rtw_ctx_variance_estimate, "rtw_ctx_variance_estimate", (self._h,), self._on_device, moments, length, depth,
                              normal, ids, min_history, radius, sigma_depth, sigma_normal, same_object, out)

    def svgf_filter(self, frame, variance, depth=None, normal=None, ids=None, albedo=None, emitted=None, levels: int = SVGF_DEFAULTS["levels"],
                    sigma_color: float = SVGF_DEFAULTS["sigma_color"], sigma_depth: float = SVGF_DEFAULTS["sigma_depth"],
                    sigma_normal: float = SVGF_DEFAULTS["sigma_normal"], same_object: bool = True,
                    albedo_floor: float = SVGF_DEFAULTS["albedo_floor"], sigma_luminance: float = SVGF_DEFAULTS["sigma_luminance"],
                    epsilon: float = SVGF_DEFAULTS["epsilon"], prefilter: bool = SVGF_DEFAULTS["prefilter"], out=None, out_variance=None):
        """The a-trous filter steered by a per-pixel variance on this context's GPU (rtw_ctx_svgf_filter, include/rtw.h): atrous_filter
        with one more term in every tap's exponent, dl^2 / (2 sigma_luminance^2 vbar + epsilon) with dl the luminance difference and vbar
        the centre's variance (its 3 x 3 Gaussian mean with prefilter), and the variance [h][w] filtered along by the squared weights.
        variance: what variance_estimate returns.  Everything else, arrays and tensors included, as atrous_filter; sigma_luminance 0 gives
        its bytes.  `out`, `out_variance`: None -> new arrays or tensors like `frame`; out may be `frame`, out_variance must be a buffer of
        its own.  Returns (out, out_variance, RtwFilterStats)."""
        return _svgf_call(lib().rtw_ctx_svgf_filter, "rtw_ctx_svgf_filter", (self._h,), self._on_device, frame, variance, depth, normal, ids,
                          albedo, emitted, levels, sigma_color, sigma_depth, sigma_normal, same_object, albedo_floor, sigma_luminance, epsilon,
                          prefilter, out, out_variance)

    def render(self, cam: RtwCamera, params: RtwParams, out=None):
        """Render into `out`: None -> new numpy array; numpy array -> host buffer; int -> raw device pointer
        (e.g. torch_tensor.data_ptr()) of [rows][width][3] f32.  Returns (out, RtwStats)."""
        rows = lib().rtw_part_rows(params.height, params.row_block, params.part_index, params.part_count)
        st = RtwStats()
        if out is None:
            out = np.empty((rows, params.width, 3), np.float32)
        if isinstance(out, np.ndarray):
            assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.size == rows * params.width * 3
            ptr = C.c_void_p(out.ctypes.data)
        else:
            ptr = C.c_void_p(int(out))
        _check(lib().rtw_ctx_render(self._h, C.byref(cam), C.byref(params), ptr, C.byref(st)), "rtw_ctx_render")
        return out, st


class MultiRenderer:
    """`rtw_mgpu`: one frame over several GPUs of a node from ONE process -- the fork / ordered join of the reference's row
    tasks (Rust/src/viewport.rs:236-244).  `devices` are HIP ordinals and may repeat."""

    def __init__(self, devices: Sequence[int]):
        self._h = C.c_void_p()
        self.n = len(devices)
        arr = (C.c_int * max(1, self.n))(*[int(d) for d in devices])
        _check(lib().rtw_mgpu_create(arr, self.n, C.byref(self._h)), "rtw_mgpu_create")
        self._scene = None

    def close(self):
        if self._h:
            lib().rtw_mgpu_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, scene: Scene, t_begin: float = 0.0, t_end: float = 0.0):
        self._scene = scene
        _check(lib().rtw_mgpu_set_scene(self._h, C.byref(scene.pod), float(t_begin), float(t_end)), "rtw_mgpu_set_scene")
        nz = scene.noise_pods()
        if nz is not None:
            _check(lib().rtw_mgpu_set_texture_noise(self._h, *nz), "rtw_mgpu_set_texture_noise")
        if scene.n_triangles:
            _check(lib().rtw_mgpu_set_triangles(self._h, scene.triangles, scene.n_triangles), "rtw_mgpu_set_triangles")

    def set_triangles(self, triangles=None):
        """rtw_mgpu_set_triangles on every device (None: clear them)."""
        if triangles is None or len(triangles) == 0:
            _check(lib().rtw_mgpu_set_triangles(self._h, None, 0), "rtw_mgpu_set_triangles")
            return
        self._tris = _triangle_array(triangles)
        _check(lib().rtw_mgpu_set_triangles(self._h, *self._tris), "rtw_mgpu_set_triangles")

    def set_lights(self, lights=None, biased_weight: float = 100.0):
        """rtw_mgpu_set_lights on every device (None: clear them)."""
        arr, n = _light_array(lights)
        _check(lib().rtw_mgpu_set_lights(self._h, arr, n, float(biased_weight)), "rtw_mgpu_set_lights")

    def set_instance_rotations(self, quats=None):
        """rtw_mgpu_set_instance_rotations on every device (None: clear them)."""
        ptr, n, _keep = _quat_array(quats)
        _check(lib().rtw_mgpu_set_instance_rotations(self._h, ptr, n), "rtw_mgpu_set_instance_rotations")

    def set_mesh_instances(self, placements=None):
        """rtw_mgpu_set_mesh_instances: Renderer.set_mesh_instances for every context (checked against all before any is touched)."""
        arr, n = _placement_array(placements)
        _check(lib().rtw_mgpu_set_mesh_instances(self._h, arr, n), "rtw_mgpu_set_mesh_instances")

    def set_option(self, key: int, value: float):
        _check(lib().rtw_mgpu_set_option(self._h, int(key), float(value)), "rtw_mgpu_set_option")

    def render(self, cam: RtwCamera, params: RtwParams, out=None):
        """Full frame into `out` (None -> new numpy array; numpy array; int -> raw device pointer).
        Returns (out, total RtwStats, [per-device RtwStats])."""
        if out is None:
            out = np.empty((params.height, params.width, 3), np.float32)
        if isinstance(out, np.ndarray):
            assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.size == params.height * params.width * 3
            ptr = C.c_void_p(out.ctypes.data)
        else:
            ptr = C.c_void_p(int(out))
        per = (RtwStats * max(1, self.n))()
        tot = RtwStats()
        _check(lib().rtw_mgpu_render(self._h, C.byref(cam), C.byref(params), ptr, per, C.byref(tot)), "rtw_mgpu_render")
        return out, tot, list(per)[: self.n]


def default_view(which: int):
    cam, p = RtwCamera(), RtwParams()
    _check(lib().rtw_scene_default_view(which, C.byref(cam), C.byref(p)), "rtw_scene_default_view")
    return cam, p


def quantize_u8(img: np.ndarray) -> np.ndarray:
    """write_img_f32's 8-bit rule (Rust/src/write_img.rs:11-15)."""
    a = np.ascontiguousarray(img, np.float32)
    out = np.empty(a.shape, np.uint8)
    lib().rtw_quantize_u8(a.ctypes.data_as(C.POINTER(C.c_float)), a.size, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out


def camera2_new(aspect, origin, vup, direction, vfov, lens_radius) -> RtwCamera:
    """Rust2 `Camera::new` (Rust2/src/viewport/camera.rs:19-53), for SAMPLER_CENTRES."""
    cam = RtwCamera()
    _check(lib().rtw_camera2_new(float(aspect), _fptr(_f3(origin)), _fptr(_f3(vup)), _fptr(_f3(direction)), float(vfov),
                                 float(lens_radius), C.byref(cam)), "rtw_camera2_new")
    return cam


def quantize_u8_rust2(img: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(img, np.float32)
    out = np.empty(a.shape, np.uint8)
    lib().rtw_quantize_u8_rust2(a.ctypes.data_as(C.POINTER(C.c_float)), a.size, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out


def _pixel_format(img: np.ndarray) -> int:
    if img.dtype == np.uint8:
        return PIXELS_U8
    if img.dtype == np.float32:
        return PIXELS_F32_RUST2
    raise ValueError(f"bilateral_filter: dtype {img.dtype}, expected uint8 or float32")


def _filter_source(what, img, shape, in_format):
    """(pointer, w, h, format, the array kept alive) of a filter's image argument: a numpy array, or a device pointer with shape + format."""
    if isinstance(img, np.ndarray):
        fmt = _pixel_format(img) if in_format is None else int(in_format)
        a = np.ascontiguousarray(img, np.uint8 if fmt == PIXELS_U8 else np.float32)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"{what}: image of shape {a.shape}, expected [h][w][3]")
        return C.c_void_p(a.ctypes.data), a.shape[1], a.shape[0], fmt, a
    if shape is None or in_format is None:
        raise ValueError(f"{what}: a device pointer needs shape=(h, w) and in_format")
    h, w = (int(v) for v in shape)
    return C.c_void_p(int(img)), w, h, int(in_format), None


def _filter_out(out, h, w):
    """(out, pointer) of a filter's `out` argument: None -> a new numpy uint8 array, a numpy array -> host buffer, int -> device pointer."""
    if out is None:
        out = np.empty((h, w, 3), np.uint8)
    if isinstance(out, np.ndarray):
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.size == h * w * 3
        return out, C.c_void_p(out.ctypes.data)
    return out, C.c_void_p(int(out))


def bilateral_filter(img: np.ndarray, size: int, proximity: int = PROXIMITY_SQUARE, avg_gradient: float = 0.0):
    """Rust2's `bilateral_filter(img, Proximity::new(size, proximity))` (Rust2/src/postprocessing.rs:70-131) on the host
    (rtw_bilateral_filter), bit for bit.  img: [h][w][3] uint8, or float32 quantised first as quantize_u8_rust2.  avg_gradient 0 computes
    the range term as the reference does; a positive value is used as given.  Returns (uint8 [h][w][3], RtwFilterStats)."""
    src, w, h, fmt, _keep = _filter_source("bilateral_filter", np.asarray(img), None, None)
    out, dst = _filter_out(None, h, w)
    st = RtwFilterStats()
    prm = RtwBilateral(int(size), int(proximity), fmt, float(avg_gradient))
    _check(lib().rtw_bilateral_filter(src, w, h, C.byref(prm), dst, C.byref(st)), "rtw_bilateral_filter")
    return out, st


def _guide_pointers(h, w, depth, normal, ids):
    """The three guide arguments as pointers: numpy arrays are shape-checked against the image, ints are device pointers, None is NULL."""
    keep, ptrs = [], []
    for name, g, dtype, shp in (("depth", depth, np.float32, (h, w)), ("normal", normal, np.float32, (h, w, 3)), ("ids", ids, np.int32, (h, w))):
        if g is None:
            ptrs.append(None)
        elif isinstance(g, np.ndarray):
            if g.shape != shp:
                raise ValueError(f"guided_filter: {name} of shape {g.shape}, expected {shp}")
            a = np.ascontiguousarray(g, dtype)
            keep.append(a)
            ptrs.append(C.c_void_p(a.ctypes.data))
        else:
            ptrs.append(C.c_void_p(int(g)))
    return ptrs, keep


def guided_filter(img: np.ndarray, size: int, depth=None, normal=None, ids=None, sigma_depth: float = 0.0, sigma_normal: float = 0.0,
                  same_object: bool = False, proximity: int = PROXIMITY_SQUARE, avg_gradient: float = 0.0):
    """The guided filter on the host (rtw_guided_filter), the bytes of Renderer.guided_filter: bilateral_filter with each tap's weights
    multiplied by the guide weight of depth [h][w] / normal [h][w][3] / ids [h][w] (include/rtw.h).  Returns (uint8 [h][w][3], RtwFilterStats)."""
    src, w, h, fmt, _keep = _filter_source("guided_filter", np.asarray(img), None, None)
    guides, _keep_g = _guide_pointers(h, w, depth, normal, ids)
    out, dst = _filter_out(None, h, w)
    st = RtwFilterStats()
    prm = RtwGuidedFilter(RtwBilateral(int(size), int(proximity), fmt, float(avg_gradient)), float(sigma_depth), float(sigma_normal),
                          int(same_object))
    _check(lib().rtw_guided_filter(src, w, h, *guides, C.byref(prm), dst, C.byref(st)), "rtw_guided_filter")
    return out, st


def _atrous_pointer(name, a, dtype, shape, on_device, keep, writable=False, who="atrous_filter"):
    """The pointer of one a-trous (or temporal) argument: None -> NULL; a torch tensor on the context's device, in place; a numpy array,
    shape-checked."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        import torch
        tdt = torch.float32 if dtype == np.float32 else torch.int32
        if on_device is None or not on_device(a, tdt) or tuple(a.shape) != shape:
            raise ValueError(f"{who}: {name} must be a contiguous {tdt} tensor of shape {shape} on the context's device")
        keep.append(a)
        return C.c_void_p(int(a.data_ptr()))
    if writable:
        if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags["C_CONTIGUOUS"] and a.shape == shape):
            raise ValueError(f"{who}: {name} must be a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
        return C.c_void_p(a.ctypes.data)
    b = np.ascontiguousarray(a, dtype)
    if b.shape != shape:
        raise ValueError(f"{who}: {name} of shape {b.shape}, expected {shape}")
    keep.append(b)
    return C.c_void_p(b.ctypes.data)


def _atrous_arguments(frame, depth, normal, ids, albedo, emitted, on_device):
    """(the C call's arguments from `in` to `emitted`, h, w, what they keep alive)."""
    shp = tuple(frame.shape) if hasattr(frame, "shape") else np.shape(frame)
    if len(shp) != 3 or shp[2] != 3:
        raise ValueError(f"atrous_filter: frame of shape {shp}, expected [h][w][3]")
    h, w = int(shp[0]), int(shp[1])
    keep = []
    ptr = lambda name, a, dtype, shape: _atrous_pointer(name, a, dtype, shape, on_device, keep)
    args = [ptr("frame", frame, np.float32, (h, w, 3)), w, h, ptr("depth", depth, np.float32, (h, w)), ptr("normal", normal, np.float32, (h, w, 3)),
            ptr("ids", ids, np.int32, (h, w)), ptr("albedo", albedo, np.float32, (h, w, 3)), ptr("emitted", emitted, np.float32, (h, w, 3))]
    return args, h, w, keep


def _atrous_params(levels, sigma_color, sigma_depth, sigma_normal, same_object, albedo_floor, depth, normal, ids) -> RtwAtrous:
    """RtwAtrous of the Python calls: a term whose guide is None is off."""
    return RtwAtrous(int(levels), float(sigma_color), float(sigma_depth) if depth is not None else 0.0,
                     float(sigma_normal) if normal is not None else 0.0, int(bool(same_object) and ids is not None), float(albedo_floor))


def atrous_filter(frame, depth=None, normal=None, ids=None, albedo=None, emitted=None, levels: int = ATROUS_DEFAULTS["levels"],
                  sigma_color: float = ATROUS_DEFAULTS["sigma_color"], sigma_depth: float = ATROUS_DEFAULTS["sigma_depth"],
                  sigma_normal: float = ATROUS_DEFAULTS["sigma_normal"], same_object: bool = True,
                  albedo_floor: float = ATROUS_DEFAULTS["albedo_floor"], out=None):
    """The a-trous filter on the host (rtw_atrous_filter), the bytes of Renderer.atrous_filter; numpy arrays only.  `out`: None -> a new
    array, or a C-contiguous float32 array [h][w][3], which may be `frame` itself.  Returns (out, RtwFilterStats)."""
    args, h, w, _keep = _atrous_arguments(frame, depth, normal, ids, albedo, emitted, None)
    if out is None:
        out = np.empty((h, w, 3), np.float32)
    _atrous_pointer("out", out, np.float32, (h, w, 3), None, _keep, writable=True)
    prm = _atrous_params(levels, sigma_color, sigma_depth, sigma_normal, same_object, albedo_floor, depth, normal, ids)
    st = RtwFilterStats()
    _check(lib().rtw_atrous_filter(*args, C.byref(prm), C.c_void_p(out.ctypes.data), C.byref(st)), "rtw_atrous_filter")
    return out, st


def _motion_pointer(motion, on_device, keep, who):
    """(pointer, n_rows) of temporal_accumulate's motion argument."""
    if hasattr(motion, "data_ptr"):
        if on_device is None or not on_device(motion) or motion.dim() != 2 or motion.shape[1] != 32 or motion.shape[0] == 0:
            raise ValueError(f"{who}: motion must be a contiguous float32 tensor of shape [n][32] on the context's device")
        keep.append(motion)
        return C.c_void_p(int(motion.data_ptr())), int(motion.shape[0])
    a = np.asarray(motion)
    if a.dtype == MOTION_ROW and a.ndim == 1:
        b = np.ascontiguousarray(a)
    elif a.ndim == 2 and a.shape[1] == 32 and a.dtype == np.float32:
        b = np.ascontiguousarray(a)
    else:
        raise ValueError(f"{who}: motion must be rows of MOTION_ROW or a float32 array of shape [n][32]")
    if len(b) == 0:
        raise ValueError(f"{who}: motion holds no row")
    keep.append(b)
    return C.c_void_p(b.ctypes.data), len(b)


def _temporal_call(fn, fn_name, head, on_device, cur, cam, depth, normal, ids, history, out_color, params, motion=None, motion_first=0,
                   out_prev_xy=None, fn_motion=None, prev_point=None, carried_normal=None, fn_points=None, hist_lo=None, hist_hi=None,
                   out_clipped=None, fn_bounded=None):
    """rtw_temporal_accumulate / rtw_ctx_temporal_accumulate from the Python arguments of temporal_accumulate: (history, variance, stats).
    With motion or out_prev_xy: fn_motion, the call with moving objects.  With prev_point or carried_normal: fn_points.  With hist_lo,
    hist_hi or out_clipped: fn_bounded."""
    who = "temporal_accumulate"
    unknown = set(params) - set(TEMPORAL_DEFAULTS) - {"offset"}
    if unknown:
        raise TypeError(f"{who}: unknown arguments {sorted(unknown)}")
    q = dict(TEMPORAL_DEFAULTS, **params)
    offset = q.get("offset", (0.5, 0.5))
    shp = tuple(cur.shape) if hasattr(cur, "shape") else np.shape(cur)
    if len(shp) != 3 or shp[2] != 3:
        raise ValueError(f"{who}: cur of shape {shp}, expected [h][w][3]")
    h, w = int(shp[0]), int(shp[1])
    keep = []
    ptr = lambda name, a, dtype, shape, writable=False: _atrous_pointer(name, a, dtype, shape, on_device, keep, writable, who)
    hist = history or {}
    prev_cam = hist.get("cam")
    if hasattr(cur, "data_ptr"):
        import torch
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=cur.device)
    else:
        new = lambda *shape: np.empty(shape, np.float32)
    out = dict(color=new(h, w, 3) if out_color is None else out_color, moments=new(h, w, 2), len=new(h, w), depth=depth, normal=normal, idx=ids,
               cam=RtwCamera.from_buffer_copy(cam))
    variance = new(h, w)
    prm = RtwTemporal(float(q["alpha"]), float(q["alpha_moments"]), int(q["max_history"]), float(q["depth_tol"]) if depth is not None else 0.0,
                      float(q["normal_cos"]) if normal is not None else 0.0, int(bool(q["same_object"]) and ids is not None),
                      (C.c_float * 2)(float(offset[0]), float(offset[1])))
    args = [ptr("cur", cur, np.float32, (h, w, 3)), w, h, C.byref(cam), ptr("depth", depth, np.float32, (h, w)),
            ptr("normal", normal, np.float32, (h, w, 3)), ptr("ids", ids, np.int32, (h, w)),
            C.byref(prev_cam) if prev_cam is not None else None,
            ptr("history color", hist.get("color"), np.float32, (h, w, 3)), ptr("history moments", hist.get("moments"), np.float32, (h, w, 2)),
            ptr("history len", hist.get("len"), np.float32, (h, w)), ptr("history depth", hist.get("depth"), np.float32, (h, w)),
            ptr("history normal", hist.get("normal"), np.float32, (h, w, 3)), ptr("history idx", hist.get("idx"), np.int32, (h, w)),
            C.byref(prm), ptr("out_color", out["color"], np.float32, (h, w, 3), True), ptr("moments", out["moments"], np.float32, (h, w, 2), True),
            ptr("len", out["len"], np.float32, (h, w), True), ptr("variance", variance, np.float32, (h, w), True)]
    st = RtwFilterStats()
    bounded = hist_lo is not None or hist_hi is not None or (out_clipped is not None and out_clipped is not False)
    points = prev_point is not None or carried_normal is not None or bounded
    if motion is None and out_prev_xy is None and not motion_first and not points:
        _check(fn(*head, *args, C.byref(st)), fn_name)
        return out, variance, st
    rows, n_rows = (None, 0) if motion is None else _motion_pointer(motion, on_device, keep, who)
    if out_prev_xy is not None and out_prev_xy is not False:
        out["prev_xy"] = new(h, w, 2) if out_prev_xy is True else out_prev_xy
    args[15:15] = [rows, n_rows, int(motion_first)]
    args.append(ptr("out_prev_xy", out.get("prev_xy"), np.float32, (h, w, 2), True))
    if not points:
        _check(fn_motion(*head, *args, C.byref(st)), fn_name + "_motion")
        return out, variance, st
    args[18:18] = [ptr("prev_point", prev_point, np.float32, (h, w, 3)), ptr("carried_normal", carried_normal, np.float32, (h, w, 3))]
    if not bounded:
        _check(fn_points(*head, *args, C.byref(st)), fn_name + "_points")
        return out, variance, st
    if out_clipped is not None and out_clipped is not False:
        out["clipped"] = new(h, w) if out_clipped is True else out_clipped
    args[20:20] = [ptr("hist_lo", hist_lo, np.float32, (h, w, 3)), ptr("hist_hi", hist_hi, np.float32, (h, w, 3))]
    args.append(ptr("out_clipped", out.get("clipped"), np.float32, (h, w), True))
    _check(fn_bounded(*head, *args, C.byref(st)), fn_name + "_bounded")
    return out, variance, st


def temporal_accumulate(cur, cam: RtwCamera, depth, normal=None, ids=None, history=None, out_color=None, motion=None, motion_first: int = 0,
                        out_prev_xy=None, prev_point=None, carried_normal=None, hist_lo=None, hist_hi=None, out_clipped=None, **params):
    """The temporal accumulation on the host (rtw_temporal_accumulate, with motion or out_prev_xy rtw_temporal_accumulate_motion, with
    prev_point or carried_normal rtw_temporal_accumulate_points, with hist_lo, hist_hi or out_clipped rtw_temporal_accumulate_bounded), the
    bytes of Renderer.temporal_accumulate; numpy arrays only.  Arguments and result as there."""
    return _temporal_call(lib().rtw_temporal_accumulate, "rtw_temporal_accumulate", (), None, cur, cam, depth, normal, ids, history, out_color, params,
                          motion, motion_first, out_prev_xy, lib().rtw_temporal_accumulate_motion, prev_point, carried_normal,
                          lib().rtw_temporal_accumulate_points, hist_lo, hist_hi, out_clipped, lib().rtw_temporal_accumulate_bounded)


def _bounds_call(fn, fn_name, head, on_device, frame, ids, radius, k, same_object, exclude_centre, out_lo, out_hi, out_clamped):
    """rtw_colour_bounds / rtw_ctx_colour_bounds from the Python arguments of colour_bounds: (lo, hi, clamped or None, stats)."""
    who = "colour_bounds"
    shp = tuple(frame.shape) if hasattr(frame, "shape") else np.shape(frame)
    if len(shp) != 3 or shp[2] != 3:
        raise ValueError(f"{who}: frame of shape {shp}, expected [h][w][3]")
    h, w = int(shp[0]), int(shp[1])
    keep = []
    ptr = lambda name, a, dtype, shape, writable=False: _atrous_pointer(name, a, dtype, shape, on_device, keep, writable, who)
    if hasattr(frame, "data_ptr"):
        import torch
        new = lambda: torch.empty((h, w, 3), dtype=torch.float32, device=frame.device)
    else:
        new = lambda: np.empty((h, w, 3), np.float32)
    out_lo = new() if out_lo is None else out_lo
    out_hi = new() if out_hi is None else out_hi
    out_clamped = None if out_clamped is None or out_clamped is False else (new() if out_clamped is True else out_clamped)
    prm = RtwColourBounds(int(radius), float(k), int(bool(same_object)), int(bool(exclude_centre)))
    st = RtwFilterStats()
    _check(fn(*head, ptr("frame", frame, np.float32, (h, w, 3)), w, h, ptr("ids", ids, np.int32, (h, w)), C.byref(prm),
              ptr("out_lo", out_lo, np.float32, (h, w, 3), True), ptr("out_hi", out_hi, np.float32, (h, w, 3), True),
              ptr("out_clamped", out_clamped, np.float32, (h, w, 3), True), C.byref(st)), fn_name)
    return out_lo, out_hi, out_clamped, st


def colour_bounds(frame, ids=None, radius: int = BOUNDS_DEFAULTS["radius"], k: float = BOUNDS_DEFAULTS["k"], same_object: bool = False,
                  exclude_centre: bool = False, out_lo=None, out_hi=None, out_clamped=None):
    """The neighbourhood colour bounds on the host (rtw_colour_bounds), the bytes of Renderer.colour_bounds; numpy arrays only.  Arguments
    and result as there."""
    return _bounds_call(lib().rtw_colour_bounds, "rtw_colour_bounds", (), None, frame, ids, radius, k, same_object, exclude_centre, out_lo, out_hi,
                        out_clamped)


def _upsample_call(fn, fn_name, head, on_device, frame_lo, size, lo, hi, scale, radius, sigma_depth, sigma_normal, same_object, albedo_floor,
                   out, out_wsum):
    """rtw_upsample_filter / rtw_ctx_upsample_filter from the Python arguments of upsample_filter: (out, wsum or None, stats)."""
    who = "upsample_filter"
    shp = tuple(frame_lo.shape) if hasattr(frame_lo, "shape") else np.shape(frame_lo)
    if len(shp) != 3 or shp[2] != 3:
        raise ValueError(f"{who}: frame_lo of shape {shp}, expected [h_lo][w_lo][3]")
    h_lo, w_lo = int(shp[0]), int(shp[1])
    w, h = int(size[0]), int(size[1])
    keep = []
    ptr = lambda name, a, dtype, shape, writable=False: _atrous_pointer(name, a, dtype, shape, on_device, keep, writable, who)
    prm = RtwUpsample(int(scale), int(radius), float(sigma_depth), float(sigma_normal), int(bool(same_object)), float(albedo_floor))

    def guides(name, d, gh, gw):
        d = d or {}
        need = {"depth": prm.sigma_depth > 0.0, "normal": prm.sigma_normal > 0.0, "idx": bool(prm.same_object), "albedo": True, "emitted": True}
        shapes = {"depth": (gh, gw), "normal": (gh, gw, 3), "idx": (gh, gw), "albedo": (gh, gw, 3), "emitted": (gh, gw, 3)}
        p = {k: ptr(f"{name}[{k!r}]", d.get(k) if need[k] else None, np.int32 if k == "idx" else np.float32, shapes[k]) for k in need}
        return RtwGuides(*(p[k].value if p[k] is not None else None for k in ("depth", "normal", "idx", "albedo", "emitted")))

    g_lo, g_hi = guides("lo", lo, h_lo, w_lo), guides("hi", hi, h, w)
    if out is None:
        out = _like(frame_lo, (h, w, 3))
    out_wsum = None if out_wsum is None or out_wsum is False else (_like(frame_lo, (h, w)) if out_wsum is True else out_wsum)
    st = RtwFilterStats()
    _check(fn(*head, ptr("frame_lo", frame_lo, np.float32, (h_lo, w_lo, 3)), w_lo, h_lo, C.byref(g_lo), w, h, C.byref(g_hi), C.byref(prm),
              ptr("out", out, np.float32, (h, w, 3), True), ptr("out_wsum", out_wsum, np.float32, (h, w), True), C.byref(st)), fn_name)
    return out, out_wsum, st


def upsample_filter(frame_lo, size, lo=None, hi=None, scale: int = 2, radius: int = UPSAMPLE_DEFAULTS["radius"],
                    sigma_depth: float = UPSAMPLE_DEFAULTS["sigma_depth"], sigma_normal: float = UPSAMPLE_DEFAULTS["sigma_normal"],
                    same_object: bool = UPSAMPLE_DEFAULTS["same_object"], albedo_floor: float = UPSAMPLE_DEFAULTS["albedo_floor"], out=None,
                    out_wsum=False):
    """The guide-steered upsampling on the host (rtw_upsample_filter), the bytes of Renderer.upsample_filter; numpy arrays only.  Arguments
    and result as there."""
    return _upsample_call(lib().rtw_upsample_filter, "rtw_upsample_filter", (), None, frame_lo, size, lo, hi, scale, radius, sigma_depth,
                          sigma_normal, same_object, albedo_floor, out, out_wsum)


def _display_pointer(who, name, a, np_dtype, shape, on_device, keep, writable):
    """The pointer of one display-stage argument of any of the dtypes float32, uint8, uint32 (a tensor: int32): a torch tensor on the
    context's device, in place; a numpy array, shape-checked."""
    if hasattr(a, "data_ptr"):
        import torch
        tdt = {np.float32: torch.float32, np.uint8: torch.uint8, np.uint32: torch.int32}[np_dtype]
        if on_device is None or not on_device(a, tdt) or tuple(a.shape) != shape:
            raise ValueError(f"{who}: {name} must be a contiguous {tdt} tensor of shape {shape} on the context's device")
        keep.append(a)
        return C.c_void_p(int(a.data_ptr()))
    if writable:
        if not (isinstance(a, np.ndarray) and a.dtype == np_dtype and a.flags["C_CONTIGUOUS"] and a.shape == shape):
            raise ValueError(f"{who}: {name} must be a C-contiguous {np.dtype(np_dtype).name} array of shape {shape}")
        return C.c_void_p(a.ctypes.data)
    b = np.ascontiguousarray(a, np_dtype)
    if b.shape != shape:
        raise ValueError(f"{who}: {name} of shape {b.shape}, expected {shape}")
    keep.append(b)
    return C.c_void_p(b.ctypes.data)


def _frame_size(who, frame):
    shp = tuple(frame.shape) if hasattr(frame, "shape") else np.shape(frame)
    if len(shp) != 3 or shp[2] != 3:
        raise ValueError(f"{who}: frame of shape {shp}, expected [h][w][3]")
    return int(shp[0]), int(shp[1])


def _new_like(a, shape, np_dtype):
    """A new array of `shape`, or a tensor on a's device when `a` is a tensor (uint32 as int32 there)."""
    if hasattr(a, "data_ptr"):
        import torch
        return torch.empty(shape, dtype={np.float32: torch.float32, np.uint8: torch.uint8, np.uint32: torch.int32}[np_dtype], device=a.device)
    return np.empty(shape, np_dtype)


def _histogram_call(fn, fn_name, head, on_device, frame, out_hist, out_counts):
    """rtw_luminance_histogram / rtw_ctx_luminance_histogram from the Python arguments of luminance_histogram: (hist, counts, stats)."""
    who = "luminance_histogram"
    h, w = _frame_size(who, frame)
    keep = []
    out_hist = _new_like(frame, (256,), np.uint32) if out_hist is None else out_hist
    out_counts = _new_like(frame, (2,), np.uint32) if out_counts is None else out_counts
    st = RtwFilterStats()
    _check(fn(*head, _display_pointer(who, "frame", frame, np.float32, (h, w, 3), on_device, keep, False), w, h,
              _display_pointer(who, "out_hist", out_hist, np.uint32, (256,), on_device, keep, True),
              _display_pointer(who, "out_counts", out_counts, np.uint32, (2,), on_device, keep, True), C.byref(st)), fn_name)
    return out_hist, out_counts, st


def luminance_histogram(frame, out_hist=None, out_counts=None):
    """The luminance histogram on the host (rtw_luminance_histogram), the counts of Renderer.luminance_histogram; numpy arrays only.
    Arguments and result as there."""
    return _histogram_call(lib().rtw_luminance_histogram, "rtw_luminance_histogram", (), None, frame, out_hist, out_counts)


def exposure_from_histogram(hist, prev_level=None, prev_exposure: float = 1.0, **metering):
    """The exposure a luminance histogram meters to (rtw_exposure_from_histogram, include/rtw.h; host only, double arithmetic): the mean bin
    position of the counted pixels between the low_permille darkest and the high_permille brightest, clamped to [min_level, max_level],
    moved from prev_level by `rate` (None or NaN: a first frame, no adaptation), and the exposure that maps the luminance of that level to
    `key`.  metering: METERING_DEFAULTS' keys.  hist: uint32 [256] (an int32 tensor as Renderer.luminance_histogram returns it is copied to
    the host).  With nothing counted the level is prev_level and the exposure prev_exposure (1 on a first frame).
    Returns (level: float, exposure: float, exactly a float32)."""
    unknown = set(metering) - set(METERING_DEFAULTS)
    if unknown:
        raise TypeError(f"exposure_from_histogram: unknown arguments {sorted(unknown)}")
    m = dict(METERING_DEFAULTS, **metering)
    if hasattr(hist, "data_ptr"):
        hist = hist.cpu().numpy().view(np.uint32)
    hh = np.ascontiguousarray(hist, np.uint32)
    if hh.shape != (256,):
        raise ValueError(f"exposure_from_histogram: hist of shape {hh.shape}, expected (256,)")
    prm = RtwMetering(int(m["low_permille"]), int(m["high_permille"]), float(m["key"]), float(m["rate"]), float(m["min_level"]), float(m["max_level"]))
    level, exposure = C.c_double(), C.c_float()
    _check(lib().rtw_exposure_from_histogram(hh.ctypes.data, C.byref(prm), float("nan") if prev_level is None else float(prev_level),
                                             float(prev_exposure), C.byref(level), C.byref(exposure)), "rtw_exposure_from_histogram")
    return level.value, exposure.value


def _display_params(params) -> RtwDisplay:
    unknown = set(params) - set(DISPLAY_DEFAULTS)
    if unknown:
        raise TypeError(f"display: unknown arguments {sorted(unknown)}")
    d = dict(DISPLAY_DEFAULTS, **params)
    return RtwDisplay(float(d["exposure"]), int(d["tone"]), float(d["white"]), int(d["transfer"]), float(d["gamma"]), int(d["quantise"]),
                      int(d["dither"]), int(d["out_format"]))


def _display_call(fn, fn_name, head, on_device, frame, out, params):
    """rtw_display / rtw_ctx_display from the Python arguments of display: (out, stats)."""
    who = "display"
    h, w = _frame_size(who, frame)
    prm = _display_params(params)
    if prm.out_format not in (DISPLAY_RGB8, DISPLAY_RGBA8, DISPLAY_F32):
        raise ValueError(f"{who}: out_format {prm.out_format}")
    shape, dt = {DISPLAY_RGB8: ((h, w, 3), np.uint8), DISPLAY_RGBA8: ((h, w, 4), np.uint8), DISPLAY_F32: ((h, w, 3), np.float32)}[prm.out_format]
    keep = []
    if out is None:
        out = _new_like(frame, shape, dt)
    st = RtwFilterStats()
    _check(fn(*head, _display_pointer(who, "frame", frame, np.float32, (h, w, 3), on_device, keep, False), w, h, C.byref(prm),
              _display_pointer(who, "out", out, dt, shape, on_device, keep, True), C.byref(st)), fn_name)
    return out, st


def display(frame, out=None, **params):
    """The display transform on the host (rtw_display), the bytes of Renderer.display; numpy arrays only.  Arguments and result as there."""
    return _display_call(lib().rtw_display, "rtw_display", (), None, frame, out, params)


def bloom_levels(w: int, h: int, levels: int):
    """The levels a bloom call of `levels` uses on a w x h frame (rtw_bloom_levels): [(w, h) of level 1, ...]; the chain stops early at the
    first 1 x 1 level."""
    sizes = (C.c_uint32 * (2 * BLOOM_MAX_LEVELS))()
    n = lib().rtw_bloom_levels(int(w), int(h), int(levels), sizes)
    if n == 0:
        raise ValueError(f"bloom_levels: w {w}, h {h}, levels {levels}")
    return [(int(sizes[2 * l]), int(sizes[2 * l + 1])) for l in range(n)]


def _bloom_params(params) -> RtwBloom:
    unknown = set(params) - set(BLOOM_DEFAULTS)
    if unknown:
        raise TypeError(f"bloom: unknown arguments {sorted(unknown)}")
    d = dict(BLOOM_DEFAULTS, **params)
    return RtwBloom(int(d["levels"]), float(d["threshold"]), float(d["knee"]), int(d["karis"]), float(d["spread"]), float(d["intensity"]))


def _bloom_call(fn, fn_name, head, on_device, frame, out, layer, params):
    """rtw_bloom / rtw_ctx_bloom from the Python arguments of bloom: (out, layer or None, stats)."""
    who = "bloom"
    h, w = _frame_size(who, frame)
    prm = _bloom_params(params)
    keep = []
    if out is None:
        out = _new_like(frame, (h, w, 3), np.float32)
    if layer is True:
        layer = _new_like(frame, (h, w, 3), np.float32)
    elif layer is False:
        layer = None
    # `out is frame`: one pointer for both (a numpy frame is otherwise read through a contiguous float32 copy)
    p_out = _display_pointer(who, "out", out, np.float32, (h, w, 3), on_device, keep, True)
    p_in = p_out if out is frame else _display_pointer(who, "frame", frame, np.float32, (h, w, 3), on_device, keep, False)
    p_layer = None if layer is None else _display_pointer(who, "layer", layer, np.float32, (h, w, 3), on_device, keep, True)
    st = RtwFilterStats()
    _check(fn(*head, p_in, w, h, C.byref(prm), p_out, p_layer, C.byref(st)), fn_name)
    return out, layer, st


def bloom(frame, out=None, layer=False, **params):
    """Bloom on the host (rtw_bloom), the bytes of Renderer.bloom; numpy arrays only.  Arguments and result as there."""
    return _bloom_call(lib().rtw_bloom, "rtw_bloom", (), None, frame, out, layer, params)


class DisplayTransform:
    """Python only: the display stage of a sequence.  step(frame) takes the frame's luminance histogram on the renderer's GPU, meters an
    exposure from it (adapting from the level of the step before by metering's `rate`) and runs the display transform with that exposure.
    params: DISPLAY_DEFAULTS' keys but for exposure, which is metered, and METERING_DEFAULTS' keys.  bloom: None, or a dict of
    BLOOM_DEFAULTS' keys: step then runs Renderer.bloom between metering and display, with `threshold` and `knee` divided by the metered
    exposure as float32 (they are in exposed units), and displays its result.  The bloomed frame is a new frame-sized array or tensor on
    every step (no buffer is kept between steps); an exposure so small that the divided threshold is not finite is a ValueError."""

    def __init__(self, renderer, bloom=None, **params):
        if "exposure" in params:
            raise TypeError("DisplayTransform: the exposure is metered; call Renderer.display for a fixed one")
        unknown = set(params) - set(DISPLAY_DEFAULTS) - set(METERING_DEFAULTS)
        if unknown:
            raise TypeError(f"DisplayTransform: unknown arguments {sorted(unknown)}")
        self.renderer = renderer
        self.metering = {k: v for k, v in params.items() if k in METERING_DEFAULTS}
        self.params = {k: v for k, v in params.items() if k in DISPLAY_DEFAULTS}
        if bloom is not None:
            unknown = set(bloom) - set(BLOOM_DEFAULTS)
            if unknown:
                raise TypeError(f"DisplayTransform: unknown bloom arguments {sorted(unknown)}")
            bloom = dict(BLOOM_DEFAULTS, **bloom)
        self.bloom = bloom
        self.reset()

    def reset(self):
        """Forget the level: the next step meters as a first frame."""
        self.level, self.exposure = None, 1.0

    def step(self, frame, out=None):
        """Returns (out, level, exposure, stats): Renderer.display's result for the metered exposure, the level and exposure now kept, and a
        dict of hist, counts and the two RtwFilterStats (histogram, display); with bloom its RtwFilterStats (bloom) too."""
        r = self.renderer
        hist, counts, st_h = r.luminance_histogram(frame)
        self.level, self.exposure = exposure_from_histogram(hist, prev_level=self.level, prev_exposure=self.exposure, **self.metering)
        if self.level != self.level:               # nothing counted on a first frame: still a first frame
            self.level = None
        stats = dict(hist=hist, counts=counts, histogram=st_h)
        if self.bloom is not None:
            e = np.float32(self.exposure)
            with np.errstate(all="ignore"):
                b = dict(self.bloom, threshold=float(np.float32(self.bloom["threshold"]) / e), knee=float(np.float32(self.bloom["knee"]) / e))
            if not (np.isfinite(b["threshold"]) and np.isfinite(b["knee"])):
                raise ValueError(f"DisplayTransform: the metered exposure {self.exposure} is too small for bloom's threshold in exposed units")
            frame, _, stats["bloom"] = r.bloom(frame, **b)
        out, st_d = r.display(frame, out=out, exposure=self.exposure, **self.params)
        stats["display"] = st_d
        return out, self.level, self.exposure, stats


def _scaled_view(cam: RtwCamera, params: RtwParams, scale: int):
    """(camera_scaled(cam, scale), a copy of params at ceil(width / scale) x ceil(height / scale))."""
    lp = RtwParams.from_buffer_copy(params)
    lp.width, lp.height = -(-params.width // scale), -(-params.height // scale)
    return camera_scaled(cam, scale), lp


class TemporalDenoiser:
    """Python only: a sequence driver around Renderer.temporal_accumulate for Viewport cameras and whole frames (part_count 1).
    `params`: temporal_accumulate's keyword arguments (TEMPORAL_DEFAULTS), but for offset, which is (0.5, 0.5).  The scene is static
    from one step to the next unless `motion` says otherwise.
    scale > 1: every step renders, takes its guides, reprojects, accumulates and filters at ceil(width / scale) x ceil(height / scale)
    with camera_scaled(cam, scale) -- the history lives at that size -- then takes the guides at params' size with `cam` and upsamples
    the filtered frame with Renderer.upsample_filter (`upsample`: a dict of its keyword arguments).  scale 1: the steps' calls are what
    they were without it."""

    def __init__(self, renderer, scale: int = 1, upsample=None, **params):
        if "offset" in params:
            raise TypeError("TemporalDenoiser: the offset is (0.5, 0.5), the centre of the jittered samplers' pixel")
        if not 1 <= int(scale) <= UPSAMPLE_MAX_SCALE:
            raise ValueError(f"{type(self).__name__}: scale {scale} outside 1 .. {UPSAMPLE_MAX_SCALE}")
        self.renderer, self.params, self.history = renderer, dict(params), None
        self.scale, self.upsample = int(scale), dict(upsample or {})

    def reset(self):
        """Drop the history: the next step starts a sequence."""
        self.history = None

    def _low(self, cam, params):
        """(the camera, the params) a step works with: the caller's own at scale 1."""
        return (cam, params) if self.scale == 1 else _scaled_view(cam, params, self.scale)

    def _upsampled(self, frame, g, cam, params, stats):
        """The step's filtered linear frame at params' size: itself at scale 1; else upsampled with the output-size guides (stats gains
        guides_hi, upsample and wsum)."""
        if self.scale == 1:
            return frame
        r = self.renderer
        hi = r.surface_map(cam, params.width, params.height, params.mint, params.maxt, params.integrator, RAYS_PIXEL, (0.5, 0.5), accel=params.accel)
        frame, wsum, st_u = r.upsample_filter(frame, (params.width, params.height), lo=g, hi=hi, scale=self.scale, out_wsum=True, **self.upsample)
        stats.update(guides_hi=hi, upsample=st_u, wsum=wsum)
        return frame

    def _guides(self, cam, params, prev_ouv, prev_poses):
        """(surface_map's dict for this frame, temporal_accumulate's prev_point / carried_normal arguments): with prev_ouv the map also
        reports tri and bary, and deform_motion turns them into the pixels' previous points."""
        r = self.renderer
        deform = prev_ouv is not None
        if prev_poses is not None and not deform:
            raise ValueError("step: prev_poses goes with prev_ouv (rigid motion alone: motion=)")
        g = r.surface_map(cam, params.width, params.height, params.mint, params.maxt, params.integrator, RAYS_PIXEL, (0.5, 0.5), accel=params.accel,
                          tri=deform, bary=deform)
        if not deform:
            return g, {}
        point, normal = r.deform_motion(g["tri"], g["bary"], prev_ouv, g["idx"] if prev_poses is not None else None, prev_poses,
                                        r.mesh_instance_first() if prev_poses is not None else 0)
        return g, dict(prev_point=point, carried_normal=normal)

    def _bounded(self, cur, g, firefly, history_clamp):
        """(the frame that enters the accumulation, temporal_accumulate's hist_lo / hist_hi / out_clipped arguments, the RtwFilterStats of
        the bounds calls made): with firefly the frame is out_clamped of colour_bounds(exclude_centre=True); with history_clamp a second
        colour_bounds of that frame gives the box of the history.  Both None: (cur, {}, {}), no call."""
        r = self.renderer
        kw, stats = {}, {}
        if firefly is not None:
            _, _, cur, stats["firefly"] = r.colour_bounds(cur, radius=firefly["radius"], k=firefly["k"], exclude_centre=True, out_clamped=True)
        if history_clamp is not None:
            same = bool(history_clamp.get("same_object", False))
            lo, hi, _, stats["history_clamp"] = r.colour_bounds(cur, ids=g["idx"] if same else None, radius=history_clamp["radius"],
                                                                k=history_clamp["k"], same_object=same)
            kw = dict(hist_lo=lo, hist_hi=hi, out_clipped=True)
        return cur, kw, stats

    def step(self, cam: RtwCamera, params: RtwParams, motion=None, motion_first: int = 0, prev_ouv=None, prev_poses=None, firefly=None,
             history_clamp=None, **atrous):
        """One frame (motion, motion_first: temporal_accumulate's, the motion of the scene's objects since the previous step; prev_ouv: the
        rows the mesh had at the previous step when refit_triangles or move_mesh_instances(ouv=) deformed it since, with prev_poses, the
        previous poses, when the mesh is placed -- the step then asks surface_map for tri and bary and deform_motion for the pixels'
        previous points): params.seed is advanced by one (in `params`), the frame rendered at gamma 1, the guides taken from surface_map at the
        pixel centres, the frame accumulated onto the history, atrous_filter (keyword arguments: its own) run on the accumulated colour
        with albedo and emission, and params.gamma applied as render_denoised does.  Returns (frame, accumulated, variance, stats): frame
        the filtered [h][w][3] float32 image, accumulated the linear accumulated colour (the history's), variance [h][w], stats a dict of
        render (RtwStats), temporal and atrous (RtwFilterStats), coverage ((len > 1).mean()), and cur and guides, the rendered frame and
        surface_map's dict this step accumulated.
        firefly: None, or dict(radius, k) -- the frame that enters everything behind the render is colour_bounds' out_clamped with
        exclude_centre (stats["cur"] is then the clamped frame).  history_clamp: None, or dict(radius, k, same_object) -- colour_bounds of
        that frame bounds the reprojected history (temporal_accumulate's hist_lo / hist_hi); history["clipped"] says by how much.  stats
        gains firefly / history_clamp, the RtwFilterStats of those calls.  With both None the step makes the calls it made without them.
        With the denoiser's scale > 1 only `frame` is at params' size: accumulated, variance, cur and guides are at the low size, and stats
        gains guides_hi (surface_map's dict at params' size), upsample (RtwFilterStats) and wsum (upsample_filter's out_wsum)."""
        if params.part_count != 1:
            raise ValueError("TemporalDenoiser: whole frames only (part_count 1)")
        r = self.renderer
        params.seed = (params.seed + 1) & 0xFFFFFFFFFFFFFFFF
        out_cam, out_params = cam, params
        cam, params = self._low(cam, params)           # (the caller's own at scale 1)
        gamma = float(params.gamma)
        params.gamma = 1.0
        try:
            cur, st = r.render(cam, params)
        finally:
            params.gamma = gamma
        g, points = self._guides(cam, params, prev_ouv, prev_poses)
        cur, bounds, st_b = self._bounded(cur, g, firefly, history_clamp)
        self.history, variance, st_t = r.temporal_accumulate(cur, cam, depth=g["depth"], normal=g["normal"], ids=g["idx"], history=self.history,
                                                             motion=motion, motion_first=motion_first, offset=(0.5, 0.5), **points, **bounds,
                                                             **self.params)
        acc = self.history["color"]
        frame, st_a = r.atrous_filter(acc, depth=g["depth"], normal=g["normal"], ids=g["idx"], albedo=g["albedo"], emitted=g["emitted"], **atrous)
        st_u = {}
        frame = self._upsampled(frame, g, out_cam, out_params, st_u)
        if gamma != 1.0:
            frame = np.power(np.maximum(frame, np.float32(0.0)), np.float32(1.0 / gamma)).astype(np.float32)
        stats = dict(render=st, temporal=st_t, atrous=st_a, coverage=float((self.history["len"] > 1).mean()), cur=cur, guides=g, **st_b, **st_u)
        return frame, acc, variance, stats


def _like(a, shape):
    """A new float32 array of `shape`, or a tensor on a's device when `a` is a tensor."""
    if hasattr(a, "data_ptr"):
        import torch
        return torch.empty(shape, dtype=torch.float32, device=a.device)
    return np.empty(shape, np.float32)


def _variance_call(fn, fn_name, head, on_device, moments, length, depth, normal, ids, min_history, radius, sigma_depth, sigma_normal,
                   same_object, out):
    """rtw_variance_estimate / rtw_ctx_variance_estimate from the Python arguments of variance_estimate: (variance, stats)."""
    who = "variance_estimate"
    shp = tuple(length.shape) if hasattr(length, "shape") else np.shape(length)
    if len(shp) != 2:
        raise ValueError(f"{who}: length of shape {shp}, expected [h][w]")
    h, w = int(shp[0]), int(shp[1])
    keep = []
    ptr = lambda name, a, dtype, shape, writable=False: _atrous_pointer(name, a, dtype, shape, on_device, keep, writable, who)
    if out is None:
        out = _like(moments, (h, w))
    prm = RtwVarianceEstimate(int(min_history), int(radius), float(sigma_depth) if depth is not None else 0.0,
                              float(sigma_normal) if normal is not None else 0.0, int(bool(same_object) and ids is not None))
    args = [ptr("moments", moments, np.float32, (h, w, 2)), ptr("length", length, np.float32, (h, w)), w, h,
            ptr("depth", depth, np.float32, (h, w)), ptr("normal", normal, np.float32, (h, w, 3)), ptr("ids", ids, np.int32, (h, w)),
            C.byref(prm), ptr("out", out, np.float32, (h, w), True)]
    st = RtwFilterStats()
    _check(fn(*head, *args, C.byref(st)), fn_name)
    return out, st


def variance_estimate(moments, length, depth=None, normal=None, ids=None, min_history: int = SVGF_DEFAULTS["min_history"],
                      radius: int = SVGF_DEFAULTS["radius"], sigma_depth: float = SVGF_DEFAULTS["sigma_depth"],
                      sigma_normal: float = SVGF_DEFAULTS["sigma_normal"], same_object: bool = True, out=None):
    """The variance estimate on the host (rtw_variance_estimate), the bytes of Renderer.variance_estimate; numpy arrays only.  Arguments and
    result as there."""
    return _variance_call(lib().rtw_variance_estimate, "rtw_variance_estimate", (), None, moments, length, depth, normal, ids, min_history, radius,
                          sigma_depth, sigma_normal, same_object, out)


def _svgf_call(fn, fn_name, head, on_device, frame, variance, depth, normal, ids, albedo, emitted, levels, sigma_color, sigma_depth, sigma_normal,
               same_object, albedo_floor, sigma_luminance, epsilon, prefilter, out, out_variance):
    """rtw_svgf_filter / rtw_ctx_svgf_filter from the Python arguments of svgf_filter: (out, out_variance, stats)."""
    who = "svgf_filter"
    args, h, w, keep = _atrous_arguments(frame, depth, normal, ids, albedo, emitted, on_device)
    ptr = lambda name, a, dtype, shape, writable=False: _atrous_pointer(name, a, dtype, shape, on_device, keep, writable, who)
    args.insert(1, ptr("variance", variance, np.float32, (h, w)))
    if out is None:
        out = _like(frame, (h, w, 3))
    if out_variance is None:
        out_variance = _like(frame, (h, w))
    prm = _atrous_params(levels, sigma_color, sigma_depth, sigma_normal, same_object, albedo_floor, depth, normal, ids)
    vprm = RtwSvgf(float(sigma_luminance), float(epsilon), int(bool(prefilter)))
    st = RtwFilterStats()
    _check(fn(*head, *args, C.byref(prm), C.byref(vprm), ptr("out", out, np.float32, (h, w, 3), True),
              ptr("out_variance", out_variance, np.float32, (h, w), True), C.byref(st)), fn_name)
    return out, out_variance, st


def svgf_filter(frame, variance, depth=None, normal=None, ids=None, albedo=None, emitted=None, levels: int = SVGF_DEFAULTS["levels"],
                sigma_color: float = SVGF_DEFAULTS["sigma_color"], sigma_depth: float = SVGF_DEFAULTS["sigma_depth"],
                sigma_normal: float = SVGF_DEFAULTS["sigma_normal"], same_object: bool = True, albedo_floor: float = SVGF_DEFAULTS["albedo_floor"],
                sigma_luminance: float = SVGF_DEFAULTS["sigma_luminance"], epsilon: float = SVGF_DEFAULTS["epsilon"], prefilter: bool = SVGF_DEFAULTS["prefilter"],
                out=None, out_variance=None):
    """The variance-steered a-trous filter on the host (rtw_svgf_filter), the bytes of Renderer.svgf_filter; numpy arrays only.  Arguments
    and result as there."""
    return _svgf_call(lib().rtw_svgf_filter, "rtw_svgf_filter", (), None, frame, variance, depth, normal, ids, albedo, emitted, levels, sigma_color,
                      sigma_depth, sigma_normal, same_object, albedo_floor, sigma_luminance, epsilon, prefilter, out, out_variance)


class SvgfDenoiser(TemporalDenoiser):
    """Python only: TemporalDenoiser with the variance-steered filter stage behind the accumulation (Renderer.variance_estimate, then
    Renderer.svgf_filter) where TemporalDenoiser has the fixed a-trous filter.  `params` as there."""

    def step(self, cam: RtwCamera, params: RtwParams, min_history: int = SVGF_DEFAULTS["min_history"], radius: int = SVGF_DEFAULTS["radius"],
             motion=None, motion_first: int = 0, prev_ouv=None, prev_poses=None, firefly=None, history_clamp=None, **svgf):
        """One frame (motion, motion_first, prev_ouv, prev_poses as TemporalDenoiser.step's): rendered, its guides taken and accumulated as TemporalDenoiser.step does; variance_estimate (min_history, radius; the
        guide sigmas and same_object those of **svgf) on the new history's moments and length; svgf_filter (keyword arguments: its own) on
        the accumulated colour with albedo and emission; params.gamma applied.  Returns (frame, accumulated, variance, stats): variance is
        the estimate the filter was steered by; stats holds render, temporal, variance and svgf (RtwStats and three RtwFilterStats),
        coverage, cur, guides, and filtered_variance, the variance the filter's levels left.  firefly, history_clamp and what a scale > 1
        changes: as TemporalDenoiser.step's."""
        if params.part_count != 1:
            raise ValueError("SvgfDenoiser: whole frames only (part_count 1)")
        r = self.renderer
        params.seed = (params.seed + 1) & 0xFFFFFFFFFFFFFFFF
        out_cam, out_params = cam, params
        cam, params = self._low(cam, params)           # (the caller's own at scale 1)
        gamma = float(params.gamma)
        params.gamma = 1.0
        try:
            cur, st = r.render(cam, params)
        finally:
            params.gamma = gamma
        g, points = self._guides(cam, params, prev_ouv, prev_poses)
        cur, bounds, st_b = self._bounded(cur, g, firefly, history_clamp)
        self.history, _, st_t = r.temporal_accumulate(cur, cam, depth=g["depth"], normal=g["normal"], ids=g["idx"], history=self.history,
                                                      motion=motion, motion_first=motion_first, offset=(0.5, 0.5), **points, **bounds,
                                                      **self.params)
        acc = self.history["color"]
        guide_kw = {k: svgf[k] for k in ("sigma_depth", "sigma_normal", "same_object") if k in svgf}
        variance, st_v = r.variance_estimate(self.history["moments"], self.history["len"], depth=g["depth"], normal=g["normal"], ids=g["idx"],
                                             min_history=min_history, radius=radius, **guide_kw)
        frame, fvar, st_s = r.svgf_filter(acc, variance, depth=g["depth"], normal=g["normal"], ids=g["idx"], albedo=g["albedo"],
                                          emitted=g["emitted"], **svgf)
        st_u = {}
        frame = self._upsampled(frame, g, out_cam, out_params, st_u)
        if gamma != 1.0:
            frame = np.power(np.maximum(frame, np.float32(0.0)), np.float32(1.0 / gamma)).astype(np.float32)
        stats = dict(render=st, temporal=st_t, variance=st_v, svgf=st_s, coverage=float((self.history["len"] > 1).mean()), cur=cur, guides=g,
                     filtered_variance=fvar, **st_b, **st_u)
        return frame, acc, variance, stats


def write_img_f32(img: np.ndarray, filename: str):
    """write_img_f32 (Rust/src/write_img.rs:6-19): 8-bit RGB PNG."""
    a = np.ascontiguousarray(img, np.float32)
    _check(lib().rtw_write_png_f32(filename.encode(), a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[1], a.shape[0]), "rtw_write_png_f32")


def write_ppm(filename: str, img: np.ndarray):
    """write_ppm (C++/src/ppm_writer.cpp:3-27): P3 text."""
    a = np.ascontiguousarray(img, np.float32)
    _check(lib().rtw_write_ppm_f32(filename.encode(), a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[1], a.shape[0]), "rtw_write_ppm_f32")


def vec3_rotated(v, rot) -> np.ndarray:
    """Vec3::rotated (Rust/src/vec3.rs:161-181)."""
    out = (C.c_float * 3)()
    lib().rtw_vec3_rotated(_fptr(_f3(v)), _fptr(_f3(rot)), out)
    return np.array(list(out), np.float32)


def device_count() -> int:
    return int(lib().rtw_device_count())
