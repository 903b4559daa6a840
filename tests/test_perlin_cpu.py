"""Perlin noise of image textures (Rust/src/texture.rs:61-194) on the host: rtw_perlin_new / rtw_perlin_eval against an independent
numpy f32 restatement of the reference, bit for bit, plus the argument checks that need no GPU and the Python Scene's noise."""
import ctypes as C
import json

import numpy as np
import pytest

import rtw_amd as R

F = np.float32


# ---- numpy restatement of PerlinNoise (one f32 rounding per written operation, the reference's order) --------------------------------
def _cell(f):
    """Rust `f as isize` of a floor()ed f32 array: saturating, NaN -> 0."""
    out = np.zeros(f.shape, np.int64)
    big, small = f >= F(2.0 ** 63), f <= F(-(2.0 ** 63))
    mid = ~np.isnan(f) & ~big & ~small
    out[mid] = f[mid].astype(np.int64)
    out[big], out[small] = np.iinfo(np.int64).max, np.iinfo(np.int64).min
    return out


def ref_noise(ranvec, perm, p):
    """PerlinNoise::noise (texture.rs:154-179) + perlin_interp (:86-107); p [n][3] f32."""
    px, py, pz = (p[:, 0].astype(F), p[:, 1].astype(F), p[:, 2].astype(F))
    fx, fy, fz = np.floor(px), np.floor(py), np.floor(pz)
    u, v, w = px - fx, py - fy, pz - fz
    i, j, k = _cell(fx), _cell(fy), _cell(fz)
    uu = u * u * (F(3.0) - F(2.0) * u)
    vv = v * v * (F(3.0) - F(2.0) * v)
    ww = w * w * (F(3.0) - F(2.0) * w)
    accum = np.zeros(len(p), F)
    for di in range(2):
        for dj in range(2):
            for dk in range(2):
                # (i + di) & 255 with wrapping addition == ((i & 255) + di) & 255
                h = perm[0][((i & 255) + di) & 255].astype(np.int64) ^ perm[1][((j & 255) + dj) & 255] ^ perm[2][((k & 255) + dk) & 255]
                c = ranvec[h]
                fi, fj, fk = F(di), F(dj), F(dk)
                d = c[:, 0] * (u - fi) + c[:, 1] * (v - fj) + c[:, 2] * (w - fk)
                accum = accum + (fi * uu + (F(1.0) - fi) * (F(1.0) - uu)) * (fj * vv + (F(1.0) - fj) * (F(1.0) - vv)) * \
                    (fk * ww + (F(1.0) - fk) * (F(1.0) - ww)) * d
    return accum


def ref_turb(ranvec, perm, p, depth):
    """PerlinNoise::turb (texture.rs:181-193)."""
    accum, weight, tp = np.zeros(len(p), F), F(1.0), p.astype(F).copy()
    for _ in range(depth):
        accum = accum + weight * ref_noise(ranvec, perm, tp)
        weight = weight * F(0.5)
        tp = tp * F(2.0)
    return np.abs(accum)


def point_set(seed=7):
    """>= 10 000 random points in [-300, 300]^3, lattice points and 1 ulp either side, huge / odd magnitudes in every coordinate."""
    rng = np.random.default_rng(seed)
    pts = [rng.uniform(-300, 300, (10000, 3)).astype(F)]
    lat = rng.integers(-300, 301, (500, 3)).astype(F)
    pts += [lat, np.nextafter(lat, F(np.inf)), np.nextafter(lat, F(-np.inf))]
    specials = [1e7, -1e7, 2.0 ** 31, -(2.0 ** 31), 2.0 ** 63, -(2.0 ** 63), 1e30, -1e30]
    odd = []
    for s in specials:
        x = F(s)
        odd += [x, np.nextafter(x, F(np.inf)), np.nextafter(x, F(-np.inf))]
    odd += [F(-0.0), F(0.0), F(np.nan), F(np.inf), F(-np.inf), F(0.5), F(-0.5)]
    base = rng.uniform(-300, 300, (len(odd), 3)).astype(F)
    for axis in range(3):
        b = base.copy()
        b[:, axis] = odd
        pts.append(b)
    pts.append(np.array([[x, x, x] for x in odd], F))
    return np.concatenate(pts, axis=0)


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def perlin():
    return R.PerlinNoise(12345)


def test_noise_matches_the_reference_restatement_bitwise(perlin):
    pts = point_set()
    got = perlin.noise(pts)
    with np.errstate(all="ignore"):
        want = ref_noise(perlin.ranvec, perlin.perm, pts)
    assert got.shape == (len(pts),)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, [(pts[i].tolist(), float(got[i]), float(want[i])) for i in bad[:5]]
    # the odd inputs give what the reference gives: NaN in -> NaN out, finite huge values stay finite
    assert np.isnan(perlin.noise(np.array([np.nan, 0.5, 0.5], F)))
    assert np.isnan(perlin.noise(np.array([0.5, np.inf, 0.5], F)))
    assert np.isfinite(perlin.noise(np.array([1e30, -1e30, 2.0 ** 63], F)))


@pytest.mark.parametrize("depth", range(1, 8))
def test_turb_matches_the_reference_restatement_bitwise(perlin, depth):
    pts = point_set(seed=depth)
    with np.errstate(all="ignore"):
        want = ref_turb(perlin.ranvec, perlin.perm, pts, depth)
    assert same_bits(perlin.turb(pts, depth), want)


def test_value_and_scalar_points(perlin):
    p = np.array([1.25, -3.5, 7.75], F)
    n = perlin.noise(p)
    assert np.ndim(n) == 0
    assert same_bits(perlin.value(p), (F(1.0) + F(n)) * F(0.5))
    assert same_bits(perlin.noise(p.reshape(1, 1, 3)).reshape(-1), np.array([n], F))
    assert perlin.turb(p, 0) == 0.0


def _pcg32_tables(seed):
    """PerlinNoise::new's ranvec from the host PCG32 (XSH-RR 64/32, the scene generators' generator), restated in Python."""
    M = (1 << 64) - 1
    state, inc = 0, (54 << 1) | 1

    def nxt():
        nonlocal state
        old = state
        state = (old * 6364136223846793005 + inc) & M
        xs = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
        rot = old >> 59
        return ((xs >> rot) | (xs << ((32 - rot) & 31))) & 0xFFFFFFFF

    nxt(); state = (state + seed) & M; nxt()
    out = np.zeros((256, 3), F)
    for i in range(256):
        v = [F(nxt() >> 8) * F(1.0 / 16777216.0) * (F(1.0) - F(-1.0)) + F(-1.0) for _ in range(3)]
        length = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        out[i] = [v[0] / length, v[1] / length, v[2] / length]
    return out


def test_perlin_new_tables():
    a, b, c = R.PerlinNoise(3), R.PerlinNoise(3), R.PerlinNoise(4)
    assert bytes(a.pod) == bytes(b.pod)
    assert a.ranvec.tobytes() != c.ranvec.tobytes()
    for perm in a.perm + c.perm:                      # create_permute shuffles over an empty range: the identity
        assert np.array_equal(perm, np.arange(256))
    for t in (a, c):
        assert np.all(np.abs(t.ranvec) <= 1.0)
        lengths = np.sqrt((t.ranvec.astype(np.float64) ** 2).sum(axis=1))
        assert np.all(np.abs(lengths - 1.0) < 4 * 2.0 ** -24), lengths
    assert same_bits(a.ranvec, _pcg32_tables(3))     # Vec3::random(-1, 1).unit(), component by component


def test_argument_checks_without_a_device():
    L = R.lib()
    t = R.PerlinNoise(1)
    pts = np.zeros((4, 3), F)
    out = np.zeros(4, F)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert L.rtw_perlin_new(1, None) == -1                       # RTW_E_INVALID
    assert L.rtw_perlin_eval(None, fp(pts), 4, 0, fp(out)) == -1
    assert L.rtw_perlin_eval(C.byref(t.pod), fp(pts), 0, 0, fp(out)) == -1
    assert L.rtw_perlin_eval(C.byref(t.pod), None, 4, 0, fp(out)) == -1
    assert L.rtw_perlin_eval(C.byref(t.pod), fp(pts), 4, 0, None) == -1
    assert L.rtw_ctx_perlin_eval(None, C.byref(t.pod), fp(pts), 4, 0, fp(out)) == -1
    assert L.rtw_ctx_set_texture_noise(None, None, 0, None, 0) == -1
    assert L.rtw_mgpu_set_texture_noise(None, None, 0, None, 0) == -1
    assert L.rtw_perlin_eval(C.byref(t.pod), fp(pts), 4, 0, fp(out)) == 0


def test_abi_sizes_of_the_noise_structs():
    assert C.sizeof(R.RtwPerlin) == 3840 and C.sizeof(R.RtwTextureNoise) == 8


def test_scene_carries_the_noise_and_json_drops_it():
    img, entry = R.texture_from_color_noise((1.0, 1.0, 1.0), 0.01, seed=9)
    assert img.shape == (1, 1, 3) and entry[1] == 0.01 and isinstance(entry[0], R.PerlinNoise)
    sp = [R.Sphere.new_with_texture((0.0, -100.5, -1.0), 100.0, (1.0, 1.0, 1.0), R.SCATTER_M, 0),
          R.Sphere.new((0.0, 0.0, -1.0), 0.5, (0.8, 0.8, 0.0), R.SCATTER_M)]
    plain = R.Scene(sp, textures=[img])
    noised = R.Scene(sp, textures=[img], noise={0: entry})
    assert plain.noise == {} and noised.noise == {0: entry}
    assert plain.noise_pods() is None
    tables, n_tables, per, n_tex = noised.noise_pods()
    assert n_tables == 1 and n_tex == 1 and per[0].perlin == 0 and per[0].scale == np.float32(0.01)
    assert bytes(tables[0]) == bytes(entry[0].pod)
    assert noised.to_json() == plain.to_json()          # texture.rs:268-276: the JSON form has no noise
    assert "noise" not in json.dumps(json.loads(noised.to_json()))
    # one table shared by two textures is uploaded once; textures without an entry have none
    p = R.PerlinNoise(2)
    two = R.Scene(sp, textures=[img, np.ones((2, 2, 3), F)], noise={1: (p, 3.0)})
    tables, n_tables, per, n_tex = two.noise_pods()
    assert n_tables == 1 and n_tex == 2 and per[0].perlin == -1 and per[1].perlin == 0 and per[1].scale == 3.0
    img2, entry2 = R.texture_with_noise(np.ones((2, 3, 3)), 0.5, perlin=p)
    assert img2.dtype == np.float32 and entry2 == (p, 0.5)
    with pytest.raises(R.RtwError):
        R.Scene(sp, textures=[img], noise={3: entry}).noise_pods()
