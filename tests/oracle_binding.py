"""ctypes binding of the CPU oracle (oracle/librtw_oracle.so) and of the reference-object checker
(oracle/_ref/librtw_ref.so).  TEST INFRASTRUCTURE: imported only by tests/, __graft_entry__.smoke()
and bench.py's cpu_baseline leg."""
import ctypes as C
import os
import subprocess

import numpy as np

import rtw_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_SO = os.environ.get("RTW_ORACLE_LIB", os.path.join(ORACLE_DIR, "librtw_oracle.so"))   # override: the sanitizer build
REF_SO = os.path.join(ORACLE_DIR, "_ref", "librtw_ref.so")
REF_STATS = os.path.join(ROOT, "tests", "golden", "ref_statistical.npz")


FLAG_DEVICE_UV = 0x20000000          # RTW_ORACLE_FLAG_DEVICE_UV (rtw_oracle.h): oracle params only, never a device call


class Extras(C.Structure):
    """RtwOracleExtras (rtw_oracle.h): the triangles and the texture noise a device context carries besides the RtwScene."""
    _fields_ = [("triangles", C.POINTER(R.RtwTriangle)), ("n_triangles", C.c_uint32),
                ("perlin", C.POINTER(R.RtwPerlin)), ("n_perlin", C.c_uint32),
                ("tex_noise", C.POINTER(R.RtwTextureNoise)), ("n_tex_noise", C.c_uint32)]


class Bounce(C.Structure):
    _fields_ = [("hit", C.c_int32), ("sphere", C.c_int32), ("front_face", C.c_int32), ("cannot_refract", C.c_int32),
                ("t", C.c_float), ("ratio", C.c_float), ("normal", C.c_float * 3), ("point", C.c_float * 3),
                ("unit_dir", C.c_float * 3), ("next_dir", C.c_float * 3)]


_lib = None
_ref = None


def build():
    """gcc the oracle (and, only where /root/reference exists, the reference objects)."""
    subprocess.run(["make", "-s", "-C", ORACLE_DIR], check=True, capture_output=True)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(ORACLE_SO):
            build()
        L = C.CDLL(ORACLE_SO)
        fp = C.POINTER(C.c_float)
        L.rtw_oracle_render.argtypes = [C.POINTER(R.RtwCamera), C.POINTER(R.RtwScene), C.POINTER(R.RtwParams), fp,
                                        C.POINTER(R.RtwStats), C.c_int]
        L.rtw_oracle_viewport_new.argtypes = [C.c_uint32, C.c_float, fp, fp, fp, fp, fp, C.POINTER(R.RtwCamera), C.POINTER(C.c_uint32)]
        L.rtw_oracle_trace_ray.argtypes = [fp, fp, C.c_float, C.POINTER(R.RtwScene), C.POINTER(R.RtwParams), C.c_uint32,
                                           C.c_uint32, C.POINTER(Bounce), C.c_int, fp]
        L.rtw_oracle_rng_seed.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
        L.rtw_oracle_rng_seed.restype = None
        L.rtw_oracle_rng_next.argtypes = [C.POINTER(C.c_uint32)]
        L.rtw_oracle_rng_next.restype = C.c_float
        L.rtw_oracle_rust2_texel_index.argtypes = [C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_int]
        L.rtw_oracle_rust2_texel_index.restype = C.c_uint32
        L.rtw_oracle_sphere_uv.argtypes = [fp, C.c_size_t, C.c_int, fp]
        L.rtw_oracle_sphere_uv.restype = None
        L.rtw_oracle_rotated.argtypes = [fp, fp, fp]
        L.rtw_oracle_rotated.restype = None
        L.rtw_oracle_render_ex.argtypes = [C.POINTER(R.RtwCamera), C.POINTER(R.RtwScene), C.POINTER(Extras), C.POINTER(R.RtwParams), fp,
                                           C.POINTER(R.RtwStats), C.c_int]
        L.rtw_oracle_triangle_hits.argtypes = [C.POINTER(R.RtwTriangle), C.c_uint32, fp, C.c_uint32, C.c_float, C.c_float, fp,
                                               C.POINTER(C.c_int32)]
        L.rtw_oracle_triangle_derived.argtypes = [C.POINTER(R.RtwTriangle), C.c_uint32, fp]
        L.rtw_oracle_triangle_derived.restype = None
        L.rtw_oracle_perlin_eval.argtypes = [C.POINTER(R.RtwPerlin), fp, C.c_uint32, C.c_uint32, fp]
        _lib = L
    return _lib


def rotated(v, rot):
    out = (C.c_float * 3)()
    lib().rtw_oracle_rotated((C.c_float * 3)(*v), (C.c_float * 3)(*rot), out)
    return np.array(list(out), np.float32)


def have_ref():
    return os.path.exists(REF_SO)


def ref():
    global _ref
    if _ref is None:
        L = C.CDLL(REF_SO)
        fp = C.POINTER(C.c_float)
        L.rtw_ref_sphere_hit.argtypes = [fp, C.c_float, fp, fp, fp, C.c_float, C.c_float, C.c_uint, C.POINTER(C.c_double)]
        L.rtw_ref_camera.argtypes = [C.c_uint32, C.c_float, C.c_float, fp, fp, fp, C.c_float, C.POINTER(R.RtwCamera), C.POINTER(C.c_uint32)]
        L.rtw_ref_s_test.argtypes = [C.POINTER(C.POINTER(C.c_char)), C.POINTER(C.c_size_t), C.POINTER(C.POINTER(C.c_char)), C.POINTER(C.c_size_t)]
        L.rtw_ref_free.argtypes = [C.c_void_p]
        L.rtw_ref_free.restype = None
        L.rtw_ref_render.argtypes = [C.POINTER(R.RtwCamera), C.POINTER(R.RtwScene), C.POINTER(R.RtwParams), C.c_uint,
                                     C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        _ref = L
    return _ref


def extras(scene):
    """The RtwOracleExtras of a Scene: its triangles (scene.triangles) and its noise (scene.noise_pods()), or None when it has neither.
    The ctypes arrays are kept alive on the returned structure."""
    nz = scene.noise_pods()
    if not scene.n_triangles and nz is None:
        return None
    x = Extras()
    if scene.n_triangles:
        x.triangles, x.n_triangles = C.cast(scene.triangles, C.POINTER(R.RtwTriangle)), scene.n_triangles
    if nz is not None:
        tables, n_tables, per, n_tex = nz
        x.perlin, x.n_perlin = C.cast(tables, C.POINTER(R.RtwPerlin)), n_tables
        x.tex_noise, x.n_tex_noise = C.cast(per, C.POINTER(R.RtwTextureNoise)), n_tex
        x._keep = nz
    return x


def render(cam, scene, params, threads=8, device_uv=False, x=None):
    """rtw_oracle_render -> ([rows][W][3] f32, RtwStats).  A Scene with triangles or texture noise goes through rtw_oracle_render_ex with
    them (or with `x`, an Extras, when given); device_uv renders with RTW_ORACLE_FLAG_DEVICE_UV set on a copy of `params`."""
    rows = R.lib().rtw_part_rows(params.height, params.row_block, params.part_index, params.part_count)
    out = np.empty((rows, params.width, 3), np.float32)
    st = R.RtwStats()
    if device_uv:
        params = R.RtwParams.from_buffer_copy(params)
        params.flags |= FLAG_DEVICE_UV
    if x is None:
        x = extras(scene)
    if x is None:
        rc = lib().rtw_oracle_render(C.byref(cam), C.byref(scene.pod), C.byref(params), out.ctypes.data_as(C.POINTER(C.c_float)),
                                     C.byref(st), threads)
    else:
        rc = lib().rtw_oracle_render_ex(C.byref(cam), C.byref(scene.pod), C.byref(x), C.byref(params),
                                        out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st), threads)
    assert rc == 0, rc
    return out, st


def triangle_hits(triangles, rays, mint, maxt):
    """rtw_oracle_triangle_hits: (t [n] f32, +inf on a miss; index [n] i32, -1 on a miss), the contract of rtw_triangle_hits."""
    arr, n = R._triangle_array(triangles)
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    t = np.empty(len(r), np.float32)
    idx = np.empty(len(r), np.int32)
    rc = lib().rtw_oracle_triangle_hits(arr, n, r.ctypes.data_as(C.POINTER(C.c_float)), len(r), float(mint), float(maxt),
                                        t.ctypes.data_as(C.POINTER(C.c_float)), idx.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, rc
    return t, idx


def triangle_derived(triangles):
    """The oracle's Triangle::new of each triangle: [n][7] f32 = normal, d, w."""
    arr, n = R._triangle_array(triangles)
    out = np.empty((n, 7), np.float32)
    lib().rtw_oracle_triangle_derived(arr, n, out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def perlin_eval(perlin, points, depth=0):
    """rtw_oracle_perlin_eval: PerlinNoise::noise (depth 0) or turb(p, depth) of a PerlinNoise at points [..., 3] -> f32 [...]."""
    pts = np.ascontiguousarray(points, np.float32)
    flat = pts.reshape(-1, 3)
    out = np.empty(len(flat), np.float32)
    rc = lib().rtw_oracle_perlin_eval(C.byref(perlin.pod), flat.ctypes.data_as(C.POINTER(C.c_float)), len(flat), int(depth),
                                      out.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0, rc
    return out.reshape(pts.shape[:-1])


def trace_ray(origin, direction, time, scene, params, pixel=0, sample=0, cap=64):
    buf = (Bounce * cap)()
    rgb = (C.c_float * 3)()
    o = (C.c_float * 3)(*origin)
    d = (C.c_float * 3)(*direction)
    n = lib().rtw_oracle_trace_ray(o, d, float(time), C.byref(scene.pod), C.byref(params), pixel, sample, buf, cap, rgb)
    assert n >= 0, n
    return list(buf)[:n], np.array(list(rgb), np.float32)


def viewport_new(width, aspect, vfov=None, origin=None, direction=None, vup=None, lens_radius=None):
    cam, h = R.RtwCamera(), C.c_uint32()
    rc = lib().rtw_oracle_viewport_new(width, aspect, R._f1(vfov), R._fptr(R._f3(origin)), R._fptr(R._f3(direction)),
                                       R._fptr(R._f3(vup)), R._f1(lens_radius), C.byref(cam), C.byref(h))
    assert rc == 0
    return cam, h.value


def ref_render(cam, scene, params, rand_seed=1):
    out = np.empty((params.height, params.width, 3), np.float64)
    seg, sec = C.c_uint64(), C.c_double()
    rc = ref().rtw_ref_render(C.byref(cam), C.byref(scene.pod), C.byref(params), rand_seed,
                              out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(seg), C.byref(sec))
    assert rc == 0
    return out, seg.value, sec.value


def block_means(x):
    """6x6 block means of a 54 x 96 frame: [9][16][3] f64 (the statistical tier's unit of comparison)."""
    return np.asarray(x, np.float64)[:54, :96].reshape(9, 6, 16, 6, 3).mean(axis=(1, 3))


def ref_render_blocks(name, cam, scene, params, rand_seed):
    """(block_means, segments) of the reference's own C++ objects rendering a view of the statistical tier, as stored in
    tests/golden/ref_statistical.npz (tests/golden/make_fixtures.py); where oracle/_ref is built, the view is rendered
    again and must reproduce the stored values exactly (serial, srand(rand_seed))."""
    z = np.load(REF_STATS)
    blocks, seg = z[name + "_blocks"], int(z[name + "_segments"])
    if have_ref():
        b, s, _ = ref_render(cam, scene, params, rand_seed)
        assert s == seg and np.array_equal(block_means(b), blocks), name
    return blocks, seg
