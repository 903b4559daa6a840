"""Round-3 CPU tests: Rust2's ImageTexture::color_at rule in the oracle, the image-level check of the sample stream
(the truncated LCG against the old RXS-M-XS permuted stream), host logic of the guided unit lengths."""
import numpy as np
import pytest

import rtw_amd as R
from tests import oracle_binding as O
from tests.test_oracle_golden import flag_params


# ---- a10: Rust2's ImageTexture::color_at (Rust2/src/objects/texture.rs:94-105) ---------------------------------------------------------
def test_rust2_texel_index_known_answers():
    """Hand-computed from the reference's lines:
         let x = (x * self.width as f32) as usize; let y = (y * self.height as f32) as usize;   multiplied: self.img[x * self.width + y]
         let emmit_x = (x * self.emmit_width as f32).floor() as usize; ...                      emmited: self.emmit_img[emmit_x * self.emmit_width + emmit_y]
    -- scaled by the SIZE (Rust/ scales by size - 1) and indexed x * width + y (Rust/: y * row + x)."""
    idx = O.lib().rtw_oracle_rust2_texel_index
    # width 4, height 2 (8 texels)
    assert idx(0.3, 0.6, 4, 2, 0) == 1 * 4 + 1          # x = (1.2) as usize = 1, y = (1.2) as usize = 1  -> 5   (the Rust/ rule: floor(.3*3) + 4*floor(.6*1) = 0)
    assert idx(0.0, 0.0, 4, 2, 0) == 0
    assert idx(0.2, 0.9, 4, 2, 0) == 0 * 4 + 1          # x = 0, y = (1.8) -> 1: texel 1 -- the SECOND COLUMN of the first row in memory: transposed
    assert idx(0.26, 0.1, 4, 2, 0) == 1 * 4 + 0         # x = (1.04) -> 1, y = 0 -> 4: the first texel of the second ROW in memory
    assert idx(0.49, 0.49, 4, 2, 0) == 1 * 4 + 0
    # x * width + y leaves the 8-texel image for u >= 0.5 (x >= 2): the reference panics there (index out of bounds); clamped to the last texel
    assert idx(0.5, 0.0, 4, 2, 0) == 7 and idx(0.99, 0.99, 4, 2, 0) == 7 and idx(1.0, 1.0, 4, 2, 0) == 7
    # a square image: every (x, y) with u, v < 1 is inside; the lookup is the transpose of the row-major one
    assert idx(0.7, 0.2, 8, 8, 0) == 5 * 8 + 1          # x = (5.6) -> 5, y = (1.6) -> 1
    assert idx(0.2, 0.7, 8, 8, 0) == 1 * 8 + 5
    # the emission image: floor() before the cast -- the same index for the non-negative u, v of a sphere
    assert idx(0.7, 0.2, 8, 8, 1) == 41 and idx(0.3, 0.6, 4, 2, 1) == 5
    # negative / NaN coordinates: `as usize` saturates to 0
    assert idx(-0.5, float("nan"), 4, 2, 0) == 0


def rust2_texture_scene(emission=True):
    """One unit sphere with a 4 x 4 image (every texel a different colour) + an 8 x 8 emission image, and a small Lambertian sphere beside it."""
    w = h = 4
    img = np.zeros((h, w, 3), np.float32)
    for j in range(h):
        for i in range(w):
            img[j, i] = (0.1 + 0.2 * i, 0.1 + 0.2 * j, 0.5)
    emit = np.zeros((8, 8, 3), np.float32)
    for j in range(8):
        for i in range(8):
            emit[j, i] = (0.01 * i, 0.01 * j, 0.0)
    big = R.Sphere.new_with_texture((0.0, 0.0, -2.0), 1.0, None, R.SCATTER_M, 0)
    for k in range(3):
        big.pod.col_mod[k] = 1.0
    small = R.Sphere.with_albedo((1.6, 0.0, -1.6), 0.4, (0.8, 0.8, 0.8), R.SCATTER_M)
    scene = R.Scene([big, small], textures=[img, emit], background=(1.0, 1.0, 1.0), emission_images={0: 1} if emission else None)
    return scene, img, emit


def test_rust2_image_texture_in_the_oracle():
    """Depth 1, no random sampling: pixel = emmited + background * multiplied = the two texels the lookup chose.  The chosen texels follow
    Rust2's transposed rule -- checked against the normal of the traced ray in f64 -- and differ from what the Rust/ rule picks."""
    scene, img, emit = rust2_texture_scene()
    p = flag_params(depth=1)
    p.integrator, p.maxt = R.INTEGRATOR_RUST2, 1000.0
    flat, eflat = img.reshape(-1, 3), emit.reshape(-1, 3)
    checked = transposed_matters = 0
    rng = np.random.default_rng(5)
    for _ in range(200):
        d = np.float32([rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), -1.0])
        rec, rgb = O.trace_ray((0.0, 0.0, 0.0), d, 0.0, scene, p, 0, 0)
        if not rec or not rec[0].hit or rec[0].sphere != 0:
            continue
        n = np.float64(list(rec[0].normal))
        u = (np.arctan2(-n[2], n[0]) + np.pi) / (2 * np.pi)
        v = 1.0 - np.arccos(-n[1]) / np.pi
        if min(abs(u * 4 - round(u * 4)), abs(v * 4 - round(v * 4)), abs(u * 8 - round(u * 8)), abs(v * 8 - round(v * 8))) < 1e-3:
            continue                                                   # too close to a texel edge for an f64 re-derivation
        x, y = int(u * 4), int(v * 4)
        ex, ey = int(np.floor(u * 8)), int(np.floor(v * 8))
        want = eflat[min(ex * 8 + ey, 63)] + np.float32(1.0) * flat[min(x * 4 + y, 15)]
        assert np.array_equal(np.float32(rgb), np.float32(want)), (u, v, rgb, want)
        checked += 1
        rust1 = flat[int(np.floor(v * 3)) * 4 + int(np.floor(u * 3))]      # sphere.rs:137-138 + texture.rs:265
        transposed_matters += not np.array_equal(flat[min(x * 4 + y, 15)], rust1)
    assert checked > 100 and transposed_matters > 50
    # without an emission image the sphere's constant `emitted` is used
    scene2, _, _ = rust2_texture_scene(emission=False)
    rec, rgb = O.trace_ray((0.0, 0.0, 0.0), np.float32([0.1, 0.2, -1.0]), 0.0, scene2, p, 0, 0)
    assert rec[0].hit and any(np.array_equal(np.float32(rgb), t) for t in flat)


# ---- the sample stream at IMAGE level: truncated LCG (the product) against the RXS-M-XS permuted stream of rounds 1 - 2a -------------------
PERMUTED = 0x40000000          # RTW_ORACLE_FLAG_PERMUTED_STREAM (include/rtw_oracle.h): oracle-only, test-only


def _block_means(img):
    h, w = img.shape[0] // 8 * 8, img.shape[1] // 8 * 8
    return img[:h, :w].astype(np.float64).reshape(h // 8, 8, w // 8, 8, 3).mean(axis=(1, 3)).reshape(-1, 3)


def _ensemble(scene, cam, p, seeds, flags):
    q = R.RtwParams.from_buffer_copy(p)
    q.flags = flags
    out, seg = [], 0
    for s in seeds:
        q.seed = s
        img, st = O.render(cam, scene, q, threads=8)
        out.append(_block_means(img)); seg += st.segments
    return np.stack(out), seg


def test_truncated_lcg_and_permuted_stream_render_the_same_image():
    """VERDICT r2 item 8 / ADVICE r2: when the output permutation of the sample stream was dropped (9 % of the GPU frame, DESIGN.md "RNG") the
    evidence was stream-level only.  Here the Book-1 final scene (config 2's scene and view, 400 x 225) is rendered at 100 spp -- as ten
    independent 10-spp renders, whose spread gives the Monte-Carlo standard error of every 8 x 8 block -- with the product's stream, with the
    permuted stream, and once more with the product's stream on other seeds (the control that shows what two independent estimates of the
    SAME distribution look like).  The block means agree within the standard error exactly as the control does, there is no bias, and the
    path-length histograms agree."""
    from tests.test_oracle_golden import small_view
    scene, cam, p = small_view(R.SCENE_C2, 400, 225, 10)
    p.gamma = 1.0
    A, seg_a = _ensemble(scene, cam, p, range(1, 11), 0)
    B, seg_b = _ensemble(scene, cam, p, range(1, 11), PERMUTED)
    Cc, seg_c = _ensemble(scene, cam, p, range(11, 21), 0)
    assert not np.array_equal(A, B)                                        # the flag does select another stream

    def z(X, Y):
        se = np.sqrt(X.var(axis=0, ddof=1) / X.shape[0] + Y.var(axis=0, ddof=1) / Y.shape[0])
        ok = se > 0                                                        # (pure-sky blocks are noise-free and identical)
        assert np.array_equal(X.mean(axis=0)[~ok], Y.mean(axis=0)[~ok])
        return ((X.mean(axis=0) - Y.mean(axis=0))[ok] / se[ok]).ravel()

    z_ab, z_ac = z(A, B), z(A, Cc)
    n = z_ab.size
    assert n > 3000
    # within 4 sigma of the standard error (18 degrees of freedom per estimate: a Student tail of ~8e-4 per entry, the control shows the same)
    assert (np.abs(z_ab) > 4.0).mean() < 0.004 and (np.abs(z_ac) > 4.0).mean() < 0.004, ((np.abs(z_ab) > 4).mean(), (np.abs(z_ac) > 4).mean())
    assert np.abs(z_ab).max() < 8.0
    # the same spread as two estimates of one distribution, and no systematic offset
    rms_ab, rms_ac = np.sqrt((z_ab ** 2).mean()), np.sqrt((z_ac ** 2).mean())
    assert 0.9 < rms_ab / rms_ac < 1.1, (rms_ab, rms_ac)
    assert abs(z_ab.mean()) < 4.0 * rms_ab / np.sqrt(n) * 3.0              # (neighbouring blocks' channels are correlated: x3)
    # whole-image radiance: the mean over all blocks agrees to the ensemble's own standard error
    ga, gb = A.mean(axis=(1, 2)), B.mean(axis=(1, 2))
    assert abs(ga.mean() - gb.mean()) < 4.0 * np.sqrt(ga.var(ddof=1) / 10 + gb.var(ddof=1) / 10)
    # segments per camera ray of the three ensembles
    rays = 400 * 225 * 100
    assert abs(seg_a - seg_b) / rays < 4.0 * abs(seg_a - seg_c) / rays + 2e-3, (seg_a, seg_b, seg_c)

    # path-length histogram: with depth d a path contributes min(length, d) closest-hit queries, so segments(d) - segments(d - 1) is the number
    # of paths at least d queries long -- exact for a stream, compared between the streams as counts
    def tail_counts(flags):
        q = R.RtwParams.from_buffer_copy(p)
        q.flags, q.seed = flags, 77
        seg = [0]
        for d in range(1, 13):
            q.depth = d
            seg.append(O.render(cam, scene, q, threads=8)[1].segments)
        return np.diff(np.array(seg, dtype=np.float64))
    ta, tb = tail_counts(0), tail_counts(PERMUTED)
    assert ta[0] == tb[0] == 400 * 225 * 10                                # every path has a first query
    zt = (ta[1:] - tb[1:]) / np.sqrt(ta[1:] + tb[1:])
    assert np.abs(zt).max() < 4.0, zt


# ---- the device's lean atan2 / acos for the spherical UV (csrc/rtw_device.h atan2_plain / acos_plain) --------------------------------------
def uv_normals():
    """2 M random unit normals and the axes (float32 [n, 3]); tests/test_gpu_device_math.py holds the device's own compile against the same set."""
    rng = np.random.default_rng(3)
    v = rng.normal(size=(2_000_000, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1], [0.6, 0.8, 0], [0, 0.6, -0.8], [1e-20, 1, 1e-20], [-1e-3, -1, 1e-9],
                     [0.5, 0.5, 0.70710678], [-0.5, -0.5, 0.70710678]], dtype=np.float64)
    return np.ascontiguousarray(np.concatenate([v, axes]).astype(np.float32))


# zeros of either sign, NaN, |y| > 1, directions of denormal length
UV_SPECIAL = np.float32([[0.0, 1.0, -0.0], [-0.0, 1.0, -0.0], [0.0, -1.0, 0.0], [-0.0, -1.0, 0.0], [np.nan, 0.0, 1.0], [1.0, 2.0, 0.0],
                         [3e-42, 1.0, -4e-42], [-2e-39, 0.5, 1e-39]])


def test_lean_atan2_acos_accuracy_and_texel_choice():
    """The device computes the UV of a textured sphere (sphere.rs:132-133) with its own reductions instead of ocml's atan2f / acosf (~130 VALU
    of every SHADE step of C5).  Measured here on the oracle's operation-for-operation copy: against f64 over 2 M random unit normals (and the
    axes), atan2 <= 2.5 ulp, acos <= 1.5 ulp -- libm grade --, and the texel the reference's rule floor(u * (row - 1)) picks agrees with the
    libm path for all but a few hits per million even on a 1024-texel-wide image."""
    import ctypes as C
    n = uv_normals()
    fp = C.POINTER(C.c_float)
    out = {}
    for plain in (0, 1):
        o = np.empty((len(n), 4), np.float32)
        O.lib().rtw_oracle_sphere_uv(n.ctypes.data_as(fp), len(n), plain, o.ctypes.data_as(fp))
        out[plain] = o
    n64 = n.astype(np.float64)
    at = np.arctan2(-n64[:, 2], n64[:, 0]); ac = np.arccos(np.clip(-n64[:, 1], -1, 1))

    def ulps(got, ref):
        return np.abs(got.astype(np.float64) - ref) / np.maximum(np.spacing(np.abs(ref.astype(np.float32))).astype(np.float64), 1e-45)
    e_at, e_ac = ulps(out[1][:, 0], at), ulps(out[1][:, 1], ac)
    assert e_at.max() <= 2.5 and e_ac.max() <= 1.5, (e_at.max(), e_ac.max())
    assert e_at.mean() < 0.5 and e_ac.mean() < 0.5
    # the special values: libm's answers for zeros of either sign, NaN in, NaN out; a direction of denormal length is still a direction
    sp = UV_SPECIAL
    a, b = np.empty((len(sp), 4), np.float32), np.empty((len(sp), 4), np.float32)
    O.lib().rtw_oracle_sphere_uv(np.ascontiguousarray(sp).ctypes.data_as(fp), len(sp), 0, a.ctypes.data_as(fp))
    O.lib().rtw_oracle_sphere_uv(np.ascontiguousarray(sp).ctypes.data_as(fp), len(sp), 1, b.ctypes.data_as(fp))
    ok = ~np.isnan(a[:, 0])
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.signbit(a[ok, 0]), np.signbit(b[ok, 0]))
    np.testing.assert_allclose(b[~np.isnan(a)], a[~np.isnan(a)], rtol=3e-7, atol=1e-7)
    for size in (2, 4, 128, 1024):
        for col in (2, 3):
            a = np.floor(out[0][:, col] * np.float32(size - 1)); b = np.floor(out[1][:, col] * np.float32(size - 1))
            assert (a != b).mean() < (1e-6 if size <= 4 else 5e-5), (size, col, (a != b).mean())
