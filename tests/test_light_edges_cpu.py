"""The light build (SPEC 9) and the mixed build (SPEC 10) at their edges, without a GPU: the scenes and cases of tests/test_gpu_light_edges.py,
and the proof -- on the numpy restatement alone (tests/lights_common.py, tests/mixed_common.py) -- that every case reaches the edge it is named
after.  The restatement's multi-sample driver (lights_common.pixel_samples / resolve) is pinned first: without lights and without the mixed
flag it is the frozen oracle's RTW_INTEGRATOR_RUST2 frame bit for bit, for every sampler and samples in {1, 3, 4, 10}.

Frames are small (the restatement traces every sample in Python): 12 x 9 for the multi-sample frames, 16 x 12 elsewhere."""
import numpy as np
import pytest

import rtw_amd as R
from tests import lights_common as LC
from tests import mixed_common as MC
from tests import oracle_binding as O

F = np.float32
CAST, BIASED, RUST2 = R.INTEGRATOR_LIGHT_CAST, R.INTEGRATOR_LIGHT_BIASED, R.INTEGRATOR_RUST2
KINDS = {"sphere": R.LIGHT_SPHERE, "quad": R.LIGHT_QUAD}
W, H = 16, 12
SW, SH = 12, 9                                           # the multi-sample frames
MULTI = [(R.SAMPLER_CENTRES, 4), (R.SAMPLER_CENTRES, 9), (R.SAMPLER_ROW, 3), (R.SAMPLER_ROW, 10), (R.SAMPLER_STRATIFIED, 3),
         (R.SAMPLER_STRATIFIED, 10)]


def params(ms, w, h, integ, depth, flags=0, **kw):
    p = ms.params(w, h, integ, depth, **kw)
    p.flags = flags
    return p


def camera_for(g, sampler, w, h):
    """RTW_SAMPLER_CENTRES reads Rust2's camera, every other sampler Rust/'s."""
    return LC.camera(g, w, h) if sampler == R.SAMPLER_CENTRES else LC.camera_no_rand(g, w, h)


def light_golden():
    """The golden light scene as a MixedScene (no mixed object: the light build)."""
    ls, g = LC.golden()
    return MC.MixedScene(g["spheres"], g["quads"], ls.lights, g["background"], weight=g["biased_weight"]), g


def same(a, b):
    """Bit-equal, or NaN in both."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def lively(img):
    """At least half of the frame's pixels are finite and non-zero."""
    ok = np.isfinite(img).all(axis=2) & (img != 0).any(axis=2)
    return int(ok.sum()) * 2 >= ok.size


# ---- 1. several samples per pixel -------------------------------------------------------------------------------------------------------
def multi_sample_cases():
    """[(name, scene, g, integrator, depth, flags, sampler, samples)]: the golden light and mixed scenes under the three integrators with
    every multi-sample setting of MULTI, and RTW_FLAG_CHUNK_SUMS (which the light driver honours: it is the generic build's driver) once per
    sampler at a sample count that is not a multiple of RTW_SUM_CHUNK."""
    out = []
    for name, (ms, g), flag in (("light", light_golden(), 0), ("mixed", MC.golden(), R.FLAG_MIXED_MATERIAL)):
        for integ in (CAST, BIASED, RUST2):
            depth = g["depth_light_cast"] if integ == CAST else 5
            for sampler, samples in MULTI:
                out.append((name, ms, g, integ, depth, flag, sampler, samples))
        for sampler, samples in ((R.SAMPLER_CENTRES, 9), (R.SAMPLER_ROW, 10), (R.SAMPLER_STRATIFIED, 10)):
            out.append((name, ms, g, BIASED, 5, flag | R.FLAG_CHUNK_SUMS, sampler, samples))
    return out


def field_multi_sample():
    """The golden box with lights_common.sphere_field (60 spheres: the tree) under LIGHT_BIASED, CENTRES at 4 samples."""
    ls, g = LC.golden()
    ms = MC.MixedScene(LC.sphere_field(g), g["quads"], ls.lights, g["background"], weight=g["biased_weight"])
    return ms, g, params(ms, SW, SH, BIASED, 5, seed=6, sampler=R.SAMPLER_CENTRES, samples=4)


@pytest.mark.parametrize("samples", [1, 3, 4, 10])
@pytest.mark.parametrize("sampler", [R.SAMPLER_ROW, R.SAMPLER_STRATIFIED, R.SAMPLER_CENTRES])
def test_multi_sample_restatement_without_lights_is_the_oracle(sampler, samples):
    """No lights, no flag: both restatements' frames are the oracle's RUST2 frame bit for bit (camera draws, sample placement, the stream per
    sample, the sum and the division), with the oracle's ray and segment counts; with RTW_FLAG_CHUNK_SUMS too, which the oracle restates."""
    _, g = LC.golden()
    ls = LC.LightScene(LC.sphere_field(g, n=6), g["quads"], [], g["background"])
    ms = MC.MixedScene(LC.sphere_field(g, n=6), g["quads"], [], g["background"])
    cam = camera_for(g, sampler, SW, SH)
    if sampler == R.SAMPLER_ROW:
        cam.time0, cam.shutter = 0.25, 0.5
    for flags in (0, R.FLAG_CHUNK_SUMS):
        p = params(ls, SW, SH, RUST2, 6, flags=flags, seed=11, sampler=sampler, samples=samples)
        ref, st = O.render(cam, ls.scene, p, 4)
        assert ref.max() > 0 and st.camera_rays == SW * SH * LC.sampler_count(sampler, samples)[0]
        img, seg, info = MC.render(ms, cam, p)
        assert np.array_equal(img, ref) and seg == st.segments, (sampler, samples, flags)
        p.integrator = BIASED
        img, seg, _ = LC.render(ls, cam, p)
        assert np.array_equal(img, ref) and seg == st.segments, (sampler, samples, flags)
    if samples == 10:                                        # ... and the flag is another frame: the chunked sum is not the plain one
        p.flags = 0
        assert not np.array_equal(LC.render(ls, cam, p)[0], ref)


def test_both_restatements_agree_on_a_multi_sample_light_frame():
    ls, g = LC.golden()
    ms, _ = light_golden()
    for sampler, samples in ((R.SAMPLER_CENTRES, 4), (R.SAMPLER_STRATIFIED, 3)):
        cam = camera_for(g, sampler, SW, SH)
        p = params(ls, SW, SH, BIASED, 4, seed=2, sampler=sampler, samples=samples)
        a, seg_a, _ = LC.render(ls, cam, p)
        b, seg_b, info = MC.render(ms, cam, p)
        assert np.array_equal(a, b) and seg_a == seg_b and info["reached"].min() > 0
        p.integrator = RUST2
        assert not np.array_equal(a, O.render(cam, ls.scene, p, 4)[0])               # the lights contribute


# ---- 2. instances under lights, static and MOVING ----------------------------------------------------------------------------------------
def instance_scene(moving):
    """The golden box and its two lights, lights_common.sphere_field on its floor (moving: every third sphere of the field has a velocity), a
    rotated Lambertian box instance and a mirror box instance.  No mixed object: the light build, SPEC 9, with GEOM."""
    ls, g = LC.golden()
    sp = LC.sphere_field(g)
    rng = np.random.default_rng(12)
    for k, s in enumerate(sp[len(g["spheres"]):]):
        if moving and k % 3 == 0:
            s["velocity"] = [0.0, float(rng.uniform(0.1, 0.4)), float(rng.uniform(-0.2, 0.2))]
    boxes = [{"a": [-0.5, -0.5, -0.5], "b": [0.5, 0.5, 0.5], "material": "lambertian", "color": [0.9, 0.8, 0.3], "rotation": [0.3, 0.5, 0.0],
              "translation": [0.9, -1.2, 3.4]},
             {"a": [-0.3, -0.3, -0.3], "b": [0.3, 0.3, 0.3], "material": "mirror", "color": [0.9, 0.9, 0.9], "rotation": [0.0, 0.4, 0.2],
              "translation": [-0.9, 0.7, 3.3]}]
    return MC.MixedScene(sp, g["quads"], ls.lights, g["background"], weight=g["biased_weight"], boxes=boxes), g


def instance_cases(moving):
    """(scene, camera, [params]): LIGHT_CAST and LIGHT_BIASED; static under NO_RAND, MOVING under ROW with time0 = 0.3, shutter = 0.5."""
    ms, g = instance_scene(moving)
    cam = LC.camera_no_rand(g, W, H)
    if moving:
        cam.time0, cam.shutter = 0.3, 0.5
    sampler = R.SAMPLER_ROW if moving else R.SAMPLER_NO_RAND
    return ms, cam, [params(ms, W, H, CAST, 10, seed=4, sampler=sampler), params(ms, W, H, BIASED, 9, seed=5, sampler=sampler)]


def check_instance_info(info, moving, n_lights=2):
    assert info["inst_hits"] > 0 and info["shadow_inst"] > 0 and info["reached"].min() > 0 and len(info["reached"]) == n_lights, info
    assert (info["nonzero_time_queries"] > 0) == moving, info


@pytest.mark.parametrize("moving", [False, True])
def test_instance_scene_reaches_instances_lights_and_times(moving):
    ms, cam, ps = instance_cases(moving)
    assert not ms.has_mixed() and len(ms.boxes) == 2
    first = [LC.closest(ms, *LC.camera_ray(cam, i, j), params(ms, W, H, RUST2, 1), j * W + i) for j in range(H) for i in range(W)]
    n_top = len(ms.spheres) + len(ms.quads)
    assert {f[0] for f in first if f is not None and f[0] >= n_top} == {n_top, n_top + 1}          # both boxes are seen directly
    for p in ps:
        img, seg, info = MC.render(ms, cam, p)
        check_instance_info(info, moving)
        assert np.isfinite(img).all() and lively(img) and seg == info["path_queries"] + 2 * info["path_hits"]


# ---- 3. the light list up to RTW_MAX_LIGHTS ----------------------------------------------------------------------------------------------
HIDDEN, ZERO, MOVER = 2, 5, 10                              # indices in LIGHT_ORDER


def light_list_scene():
    """The golden box without its own lights, five emissive spheres (the last one moving: its mid-point stays at its time-0 place), a sphere
    that emits nothing, seven emissive quads, and -- behind the green wall and a two-layer blocker of its own, where no path arrives -- a hidden
    emissive sphere.  Returns (spheres, quads, the 16 entries the light lists are cut from)."""
    _, g = LC.golden()
    walls = [dict(q) for q in g["quads"] if q["name"] != "light quad"]
    lam = {"material": "lambertian", "color": [1.0, 1.0, 1.0]}
    sp = [dict(lam, origin=[-1.2, 1.0, 4.0], radius=0.25, emitted=[6.0, 5.0, 3.0]),
          dict(lam, origin=[1.1, 0.9, 3.2], radius=0.2, emitted=[2.0, 3.0, 6.0]),
          dict(lam, origin=[0.2, -1.3, 4.6], radius=0.3, emitted=[3.0, 6.0, 2.0]),
          dict(lam, origin=[-0.9, -0.8, 2.6], radius=0.15, emitted=[5.0, 5.0, 5.0]),
          dict(lam, origin=[1.3, -0.4, 4.4], radius=0.2, emitted=[4.0, 1.0, 5.0], velocity=[0.0, 0.8, -0.4]),
          dict(lam, origin=[-0.2, 0.4, 3.6], radius=0.3, emitted=[0.0, 0.0, 0.0], color=[0.8, 0.8, 0.8]),          # emits nothing
          dict(lam, origin=[0.3, 0.2, 7.0], radius=0.3, emitted=[9.0, 9.0, 9.0]),                                    # hidden
          {"origin": [0.8, -1.7, 2.4], "radius": 0.3, "material": "mirror", "color": [0.9, 0.9, 0.9], "emitted": [0.0, 0.0, 0.0]},
          {"origin": [-1.3, -1.6, 3.9], "radius": 0.35, "material": "glass", "color": [1.0, 1.0, 1.0], "emitted": [0.0, 0.0, 0.0]}]
    # (the side walls end at z = 5 and the green wall stands at z = 6, its normal towards +z: paths leave through the gap and through the
    # wall.  The blocker has two layers, normals towards -z -- Rust2's Lambertian scatters about the normal as given, so a path that hits it
    # turns back: a hit on the first layer, whose shadow ray starts on it, is stopped by the second; nothing arrives between the two or behind.)
    quads = walls + [dict(lam, origin=[-6.0, -6.0, z], u=[0.0, 12.0, 0.0], v=[12.0, 0.0, 0.0], emitted=[0.0, 0.0, 0.0], color=[0.5, 0.5, 0.5])
                     for z in (6.5, 6.6)]
    n_fixed = len(quads)
    for k in range(7):                                                                  # emissive quads about the box, facing every way
        o = [[-1.6, 1.5, 2.0], [0.9, 1.6, 4.8], [-1.9, -0.5, 3.0], [1.9, 0.3, 2.2], [-0.5, -1.9, 3.3], [0.4, 1.2, 5.6], [-1.5, -1.2, 5.2]][k]
        u, vv = [([0.4, 0, 0], [0, 0, 0.4]), ([0.3, 0, 0], [0, 0.2, 0.3]), ([0, 0.5, 0], [0, 0, 0.5]), ([0, 0, 0.4], [0, 0.4, 0]),
                 ([0.6, 0, 0], [0, 0, 0.3]), ([0.5, 0, 0], [0, 0.5, 0]), ([0.3, 0.3, 0], [0, 0, 0.3])][k]
        quads.append(dict(lam, origin=o, u=[float(x) for x in u], v=[float(x) for x in vv], emitted=[float(2 + k % 3), float(1 + k % 4), float(3 - k % 2)]))
    S, Q = R.LIGHT_SPHERE, R.LIGHT_QUAD
    order = [(Q, n_fixed), (S, 0), (S, 6), (Q, n_fixed + 1), (S, 1), (S, 5), (Q, n_fixed + 2), (S, 0), (S, 2), (Q, n_fixed + 3), (S, 4),
             (Q, n_fixed + 4), (S, 3), (Q, n_fixed), (Q, n_fixed + 5), (Q, n_fixed + 6)]
    assert len(order) == R.MAX_LIGHTS and order[HIDDEN] == (S, 6) and order[ZERO] == (S, 5) and order[MOVER] == (S, 4)
    return sp, quads, order, g


def light_list_cases(n, lights=None):
    """(scene, camera, [params]) with the first n entries of the list (n = 1: one emissive quad; 15 and 16 hold every kind): LIGHT_CAST under
    NO_RAND and LIGHT_BIASED under ROW through a shutter (the scene is MOVING: one light has a velocity)."""
    sp, quads, order, g = light_list_scene()
    ms = MC.MixedScene(sp, quads, order[:n] if lights is None else lights, g["background"], weight=20.0)
    cam = LC.camera_no_rand(g, W, H)
    cam.time0, cam.shutter = 0.2, 0.6
    return ms, cam, [params(ms, W, H, CAST, 10, seed=3), params(ms, W, H, BIASED, 5, seed=7, sampler=R.SAMPLER_ROW)]


@pytest.mark.parametrize("n", [1, 15, 16])
def test_light_list_every_light_is_reached_but_the_hidden_one(n):
    ms, cam, ps = light_list_cases(n)
    assert len(ms.lights) == n
    for p in ps:
        img, seg, info = MC.render(ms, cam, p)
        assert seg == info["path_queries"] + n * info["path_hits"] and lively(img) and np.isfinite(img).all()
        for k in range(n):
            if k == HIDDEN:
                assert info["reached"][k] == 0 and info["blocked"][k] == info["path_hits"], (n, k, info)
            else:
                assert info["reached"][k] > 0, (n, k, info)
        if p.sampler == R.SAMPLER_ROW:
            assert info["nonzero_time_queries"] > 0
    if n == 16:
        # the mover's mid-point is its place at time 0 whatever its velocity
        assert np.array_equal(ms.mids[MOVER], LC.mid_sphere(ms.spheres[4]["origin"], ms.spheres[4]["radius"]))
        assert np.array_equal(R.light_mid(ms.scene, ms.lights[MOVER]), ms.mids[MOVER])


def test_a_light_that_emits_nothing_counts_under_light_cast_only():
    """emitted = 0: the threshold is 1 / 0 = inf and LIGHT_BIASED skips the light; LIGHT_CAST adds 0 * pdf / d2 and count + 1."""
    ms, cam, ps = light_list_cases(16)
    without = [l for k, l in enumerate(ms.lights) if k != ZERO]
    ms2, _, _ = light_list_cases(15, lights=without)
    for p in ps:
        a, b = MC.render(ms, cam, p)[0], MC.render(ms2, cam, p)[0]
        assert np.array_equal(a, b) == (p.integrator == BIASED), p.integrator


# ---- 4. depth 0 and 1 --------------------------------------------------------------------------------------------------------------------
def sphere_only(mixed):
    """test_gpu_lights' / test_gpu_mixed's sphere-only scene (59 spheres, no quads), static; mixed: a mixed ground and every fourth small sphere."""
    rng = np.random.default_rng(21)
    sp = [{"origin": [0.0, -101.0, 4.0], "radius": 100.0, "material": "mixed" if mixed else "lambertian", "exp": 2.0, "color": [0.6, 0.6, 0.5],
           "emitted": [0, 0, 0]},
          {"origin": [-0.8, 0.6, 3.5], "radius": 0.25, "material": "lambertian", "color": [1, 1, 1], "emitted": [6.0, 5.0, 3.0]},
          {"origin": [1.0, 0.2, 4.5], "radius": 0.2, "material": "lambertian", "color": [1, 1, 1], "emitted": [2.0, 3.0, 6.0]}]
    for k in range(56):
        sp.append({"origin": [float(rng.uniform(-2.5, 2.5)), float(rng.uniform(-0.9, -0.3)), float(rng.uniform(2.0, 7.0))],
                   "radius": float(rng.uniform(0.08, 0.25)), "material": ["lambertian", "mirror", "glass", "mixed" if mixed else "lambertian"][k % 4],
                   "exp": float(1 + k % 7), "color": [float(x) for x in rng.uniform(0.3, 1.0, 3)], "emitted": [0.0, 0.0, 0.0]})
    return MC.MixedScene(sp, [], [(R.LIGHT_SPHERE, 1), (R.LIGHT_SPHERE, 2)], (0.05, 0.06, 0.08), weight=100.0)


def depth_cases():
    """[(name, scene, g, flags, quads?)]: golden light scene (SPEC 9, GEOM), golden mixed scene (SPEC 10, GEOM), the sphere-only scene without
    and with mixed spheres (SPEC 9 and 10 without the quad stage)."""
    _, g = LC.golden()
    return [("light", light_golden()[0], g, 0, True), ("mixed", MC.golden()[0], g, R.FLAG_MIXED_MATERIAL, True),
            ("spheres", sphere_only(False), g, 0, False), ("mixed spheres", sphere_only(True), g, R.FLAG_MIXED_MATERIAL, False)]


def depth_params(ms, flags):
    """LIGHT_CAST, LIGHT_BIASED and RUST2 plus the flag, at depth 0 and 1."""
    return [params(ms, W, H, integ, depth, flags=flags if integ != RUST2 else R.FLAG_MIXED_MATERIAL, seed=2)
            for integ in (CAST, BIASED, RUST2) for depth in (0, 1)]


def test_depth_zero_and_one_on_the_restatement():
    """LIGHT_CAST ignores depth; the other two return the background at depth 0 without a query."""
    for name, ms, g, flags, _ in depth_cases():
        cam = LC.camera_no_rand(g, W, H)
        bg = np.broadcast_to(ms.background, (H, W, 3))
        for p in depth_params(ms, flags):
            img, seg, info = MC.render(ms, cam, p)
            if p.integrator == CAST:
                q = R.RtwParams.from_buffer_copy(p)
                q.depth = 9
                ref9, seg9, _ = MC.render(ms, cam, q)
                assert np.array_equal(img, ref9) and seg == seg9 and lively(img), (name, p.depth)
            elif p.depth == 0:
                assert np.array_equal(img, bg) and seg == 0, name
            else:
                assert seg == W * H + len(ms.lights) * info["path_hits"] * (p.integrator == BIASED) and info["path_hits"] > 0, name


# ---- 5. what nothing guards ----------------------------------------------------------------------------------------------------------------
def mid_point_quad(g, z=4.0):
    """An emissive axis-aligned quad in the plane z = `z` whose mid-point (rtw_light_mid) is bit for bit the hit point P of a NO_RAND camera
    ray (camera at the origin looking down +z: d.z == 1, so P = d * z exactly): corners P -/+ (a, b) with a, b powers of two, searched over
    pixels near the frame's middle.  Returns (quad, pixel (i, j), P)."""
    cam = LC.camera_no_rand(g, W, H)
    for j in (H // 2, H // 2 - 1, H // 2 + 1):
        for i in (W // 2, W // 2 - 1, W // 2 + 1):
            o, d = LC.camera_ray(cam, i, j)
            assert d[2] == F(1.0) and not o.any()
            P = (d * F(z)).astype(F)
            for a in (0.5, 0.25):
                for b in (0.25, 0.5):
                    q = {"origin": [float(F(P[0] - F(a))), float(F(P[1] - F(b))), z], "u": [2 * a, 0.0, 0.0], "v": [0.0, 2 * b, 0.0],
                         "material": "lambertian", "color": [1.0, 1.0, 1.0], "emitted": [3.0, 2.0, 4.0]}
                    if LC.mid_quad(q["origin"], q["u"], q["v"]).tobytes() == P.tobytes():
                        return q, (i, j), P
    raise AssertionError("no pixel whose hit point is a quad's mid-point")


def first_hit(ms, cam, i, j):
    return LC.closest(ms, *LC.camera_ray(cam, i, j), params(ms, W, H, RUST2, 1), j * W + i)


def tiny_light_at(P):
    """A sphere of radius 2^-60 about P: its mid-point ((c - r) + (c + r)) * 0.5 is P, and a ray that ends at P does not hit it before."""
    return {"origin": [float(x) for x in P], "radius": 2.0 ** -60, "material": "lambertian", "color": [1.0, 1.0, 1.0], "emitted": [5.0, 4.0, 3.0]}


def mid_point_cases():
    """[(name, scene, camera, pixel, P, light index whose mid-point is P, NaN pixels expected)].

    quad / quad + sphere / quad + field: the light is a quad whose mid-point is the first hit of one pixel -- the shadow direction of that
    hit towards its own light is 0 / 0.  No quad accepts such a ray, the reference's sphere test does (NaN root): with a sphere first in the list
    the closest hit of the NaN ray is that sphere, which is not the light, so the frame stays finite; the field makes the tree kernel send the
    ray through wild_ray_query.  tiny + ...: the first sphere of the list is a light of radius 2^-60 centred on the first hit of a pixel (on
    a wall / on the ground sphere): the NaN ray's closest hit is that sphere with a NaN t, it IS the light, and NaN flows into S and the pixel."""
    _, g = LC.golden()
    cam = LC.camera_no_rand(g, W, H)
    walls = [dict(q) for q in g["quads"] if q["name"] != "light quad"]
    q, pix, P = mid_point_quad(g)
    lam = {"material": "lambertian", "color": [0.7, 0.7, 0.7], "emitted": [0.0, 0.0, 0.0]}
    ball = dict(lam, origin=[1.0, -1.0, 3.0], radius=0.4)
    lamp = {"origin": [-0.4, 0.8, 4.5], "radius": 0.2, "material": "lambertian", "color": [1.0, 1.0, 1.0], "emitted": [4.0, 2.0, 4.0]}
    out = []
    QL = [(R.LIGHT_QUAD, len(walls))]
    out.append(("quad", MC.MixedScene([], walls + [q], QL, g["background"], weight=100.0), cam, pix, P, 0, False))
    out.append(("quad + sphere", MC.MixedScene([ball, lamp], walls + [q], QL + [(R.LIGHT_SPHERE, 1)], g["background"], weight=100.0), cam, pix, P, 0, False))
    field = [ball, lamp] + LC.sphere_field(g)[1:]
    out.append(("quad + field", MC.MixedScene(field, walls + [q], QL + [(R.LIGHT_SPHERE, 1)], g["background"], weight=100.0), cam, pix, P, 0, False))
    # a tiny light on the green wall (GEOM builds), alone and with the field
    plain = MC.MixedScene([lamp], walls, [(R.LIGHT_SPHERE, 0)], g["background"])
    i, j = W // 2 + 2, H // 2 - 2
    Pw = first_hit(plain, cam, i, j)[2]
    out.append(("tiny + walls", MC.MixedScene([tiny_light_at(Pw), lamp], walls, [(R.LIGHT_SPHERE, 1), (R.LIGHT_SPHERE, 0)], g["background"],
                                              weight=100.0), cam, (i, j), Pw, 1, True))
    out.append(("tiny + walls + field", MC.MixedScene([tiny_light_at(Pw)] + field, walls, [(R.LIGHT_SPHERE, 2), (R.LIGHT_SPHERE, 0)], g["background"],
                                                      weight=100.0), cam, (i, j), Pw, 1, True))
    # the builds without quads: the tiny light on the ground sphere of the sphere-only scene (59 + 1 spheres: the tree)
    so = sphere_only(False)
    i, j = W // 2 - 3, H - 2
    Pg = first_hit(so, cam, i, j)
    assert Pg is not None and Pg[0] == 0
    sp = [tiny_light_at(Pg[2])] + so.spheres
    out.append(("tiny + spheres", MC.MixedScene(sp, [], [(R.LIGHT_SPHERE, 2), (R.LIGHT_SPHERE, 0), (R.LIGHT_SPHERE, 3)], so.background, weight=100.0),
                cam, (i, j), Pg[2], 1, True))
    return out


def mid_point_params(ms):
    return [params(ms, W, H, CAST, 10, seed=1), params(ms, W, H, BIASED, 4, seed=1)]


def test_mid_point_cases_reach_a_nan_shadow_direction():
    for name, ms, cam, (i, j), P, li, want_nan in mid_point_cases():
        h = first_hit(ms, cam, i, j)
        assert h is not None and h[2].tobytes() == np.asarray(P, F).tobytes(), name                  # the pixel's first hit is P ...
        assert ms.mids[li].tobytes() == h[2].tobytes(), name                                         # ... and P is the light's mid-point,
        assert R.light_mid(ms.scene, ms.lights[li]).tobytes() == h[2].tobytes(), name                # by the library's own rtw_light_mid
        with np.errstate(invalid="ignore", divide="ignore"):
            to = (ms.mids[li] - h[2]).astype(F)
            assert np.isnan((to / np.sqrt(LC.dot(to, to))).astype(F)).all(), name
        for p in mid_point_params(ms):
            img, seg, info = MC.render(ms, cam, p)
            nan = np.isnan(img).any(axis=2)
            assert lively(img), name
            assert bool(nan.any()) == want_nan, (name, p.integrator, int(nan.sum()))
            if want_nan:
                assert nan[j, i], (name, p.integrator)


WEIGHTS = [0.0, 1e30, float("nan"), float("inf"), -0.5, -100.0]


def weight_case(weight):
    """rtw_ctx_set_lights checks no weight: the golden light scene under LIGHT_BIASED with it, seen from two units further back and in front
    of a sky, so that the box fills a third of the frame and the rest is background whatever the weight does."""
    ls, g = LC.golden()
    g = dict(g, camera=dict(g["camera"], origin=[0.0, 0.0, -2.0]))
    ms = MC.MixedScene(g["spheres"], g["quads"], ls.lights, (0.3, 0.4, 0.5), weight=float(weight))
    return ms, LC.camera_no_rand(g, W, H), params(ms, W, H, BIASED, 9, seed=3)


def test_weights_at_and_beyond_the_edges():
    """weight 0 with emissive lights: RUST2's frame (count = 1, S = 0).  1e30: finite.  NaN, inf, -0.5 (count = 1 - 0.5 - 0.5 = 0): non-finite
    pixels wherever both lights are accepted; no weight is refused."""
    for wgt in WEIGHTS:
        ms, cam, p = weight_case(wgt)
        img, seg, info = MC.render(ms, cam, p)
        assert info["reached"].min() > 0 and lively(img), wgt
        if wgt == 0.0:
            q = R.RtwParams.from_buffer_copy(p)
            q.integrator = RUST2
            assert np.array_equal(img, O.render(cam, ms.scene, q, 4)[0])
        elif wgt == 1e30:
            assert np.isfinite(img).all()
        elif wgt == -100.0:
            assert np.isfinite(img).all() and not np.array_equal(img, MC.render(weight_case(100.0)[0], cam, p)[0])   # count = 1 - 200
        else:
            assert not np.isfinite(img).all(), wgt


def mixed_edge_scene():
    """The golden mixed scene with: a mixed sphere of exponent 0 and one of the largest finite f32; a free-standing mixed quad seen from its back
    (normal (0, 0, 1), away from the camera; the lobe is about the unflipped normal) that is also a light; and a mixed light sphere."""
    _, g = MC.golden()
    big = float(np.finfo(np.float32).max)
    sp = g["spheres"] + [
        {"origin": [1.0, -1.3, 3.4], "radius": 0.5, "material": "mixed", "exp": 0.0, "color": [0.9, 0.9, 0.6], "emitted": [0.0, 0.0, 0.0]},
        {"origin": [-1.1, -1.3, 3.0], "radius": 0.5, "material": "mixed", "exp": big, "color": [0.6, 0.9, 0.9], "emitted": [0.0, 0.0, 0.0]},
        {"origin": [1.2, 1.0, 4.2], "radius": 0.3, "material": "mixed", "exp": 2.0, "color": [1.0, 1.0, 1.0], "emitted": [3.0, 3.0, 1.0]}]
    back = {"origin": [-1.4, 0.2, 3.2], "u": [1.0, 0.0, 0.0], "v": [0.0, 1.0, 0.0], "material": "mixed", "exp": 1.0, "color": [0.8, 0.7, 0.9],
            "emitted": [1.0, 2.0, 1.0]}
    quads = g["quads"] + [back]
    lights = [(KINDS[l["kind"]], l["index"]) for l in g["lights"]] + [(R.LIGHT_QUAD, len(quads) - 1), (R.LIGHT_SPHERE, 3)]
    return MC.MixedScene(sp, quads, lights, g["background"], weight=g["biased_weight"]), g


def mixed_edge_params(ms):
    return [params(ms, W, H, integ, 10 if integ == CAST else 5, flags=R.FLAG_MIXED_MATERIAL, seed=9) for integ in (CAST, BIASED, RUST2)]


def test_mixed_exponents_at_the_ends_and_a_lobe_from_behind():
    ms, g = mixed_edge_scene()
    cam = LC.camera_no_rand(g, W, H)
    seen, back = set(), 0
    for j in range(H):
        for i in range(W):
            o, d = LC.camera_ray(cam, i, j)
            h = first_hit(ms, cam, i, j)
            if h is None:
                continue
            seen.add(h[0])
            back += int(h[0] == len(ms.spheres) + len(ms.quads) - 1 and LC.dot(d, h[3]) > 0)          # hit from behind: d . n > 0
    assert {1, 2, 3} <= seen and back > 0, (seen, back)
    p = params(ms, W, H, RUST2, 3, flags=R.FLAG_MIXED_MATERIAL)
    assert R.mixed_validate(ms.scene, p) == R.RTW_OK                                                   # both exponents are in the domain
    for p in mixed_edge_params(ms):
        img, seg, info = MC.render(ms, cam, p)
        assert info["mixed_hits"] > 0 and np.isfinite(img).all() and (lively(img) if p.integrator != RUST2 else img.max() > 0), p.integrator
        if p.integrator != RUST2:
            assert info["reached"][2] > 0 and info["reached"][3] > 0                                   # the mixed lights are reached


DIM = 0.02463994361460209      # the f32 e with 1 / (255 * e) == FRAC_1_2PI bit for bit (searched; asserted below)


def threshold_case():
    """pdf == LIGHT_BIASED's threshold exactly.  MixedMaterial::new(0)'s pdf is pow(cos, 0) * (0 + 1) * FRAC_1_2PI = FRAC_1_2PI for every shadow
    direction with cos >= 0, and a light whose largest emitted component is DIM has the threshold 1 / (255 * DIM) == FRAC_1_2PI: on the two
    mixed walls (exponent 0 here) `pdf <= threshold` skips that light where `pdf < threshold` would add it."""
    _, g = MC.golden()
    quads = [dict(q, exp=0.0) if q["material"] == "mixed" else dict(q) for q in g["quads"]]
    sp = g["spheres"] + [{"origin": [0.5, 0.6, 3.5], "radius": 0.3, "material": "lambertian", "color": [1.0, 1.0, 1.0],
                          "emitted": [DIM, DIM / 2, DIM / 4]}]
    lights = [(KINDS[l["kind"]], l["index"]) for l in g["lights"]] + [(R.LIGHT_SPHERE, 1)]
    ms = MC.MixedScene(sp, quads, lights, g["background"], weight=g["biased_weight"])
    return ms, LC.camera_no_rand(g, W, H), params(ms, W, H, BIASED, 4, flags=R.FLAG_MIXED_MATERIAL, seed=6)


def test_a_pdf_equal_to_the_threshold_is_skipped(monkeypatch):
    """On the restatement: the dim light meets pdf == threshold bit for bit at accepted shadow queries, `<=` skips it there, and the frame
    restated with `<` is another frame -- so a device that compared with `<` would not reproduce this one."""
    assert F(F(1.0) / F(F(255.0) * F(DIM))).tobytes() == MC.FRAC_1_2PI.tobytes()
    ms, cam, p = threshold_case()
    plain = LC.light_term
    equal = [0]

    def counting(biased, pdf, e, t, rd, w):
        mx = max(e[0], e[1], e[2])
        equal[0] += int(biased and F(pdf).tobytes() == F(F(1.0) / F(F(255.0) * mx)).tobytes())
        return plain(biased, pdf, e, t, rd, w)

    def strict(biased, pdf, e, t, rd, w):
        s, dc = plain(biased, pdf, e, t, rd, w)
        if s is None and biased and F(pdf) == F(F(1.0) / F(F(255.0) * max(e[0], e[1], e[2]))):
            d2 = F(F(t * t) * LC.dot(rd, rd))
            return (((e * pdf).astype(F) / d2).astype(F) * F(w)).astype(F), F(w)
        return s, dc

    monkeypatch.setattr(LC, "light_term", counting)
    img, _, info = MC.render(ms, cam, p)
    assert equal[0] > 0 and info["reached"][2] > 0 and np.isfinite(img).all() and lively(img), (equal, info)
    monkeypatch.setattr(LC, "light_term", strict)
    other = MC.render(ms, cam, p)[0]
    assert not np.array_equal(other, img)


def grazing_case():
    """A Lambertian light quad lying in the plane y = -0.1 under the camera's line of sight: the rows below the horizon skim it, and at every
    hit on it the shadow ray to its own mid-point runs in the quad's plane (cos about 0, clamped) while the other light sees it from above."""
    ms0, g = light_golden()
    flat = {"origin": [-1.8, -0.1, 1.5], "u": [3.6, 0.0, 0.0], "v": [0.0, 0.0, 3.0], "material": "lambertian", "color": [0.9, 0.9, 0.9],
            "emitted": [0.5, 0.4, 0.3]}
    quads = g["quads"] + [flat]
    ms = MC.MixedScene(g["spheres"], quads, ms0.lights + [(R.LIGHT_QUAD, len(quads) - 1)], g["background"], weight=g["biased_weight"])
    return ms, LC.camera_no_rand(g, W, 2 * H), [params(ms, W, 2 * H, CAST, 10), params(ms, W, 2 * H, BIASED, 4, seed=5)]


def test_grazing_hits_on_a_light_clamp_the_cosine():
    ms, cam, ps = grazing_case()
    obj = len(ms.spheres) + len(ms.quads) - 1
    n, clamped = 0, 0
    for j in range(2 * H):
        for i in range(W):
            o, d = LC.camera_ray(cam, i, j)
            h = LC.closest(ms, o, d, params(ms, W, 2 * H, RUST2, 1), j * W + i)
            if h is None or h[0] != obj:
                continue
            n += 1
            rd = LC.unit((ms.mids[2] - h[2]).astype(F))
            pdf = LC.material_pdf(ms.mat(obj), h[2], h[3], d, 0.0, h[2], rd, 0.0)
            clamped += int(pdf == 0.0)
            assert abs(float(LC.dot(LC.unit(d), h[3]))) < 0.1                                          # the camera ray itself grazes the quad
    assert n >= W and clamped == n, (n, clamped)                                                       # the cosine clamps to 0 at every one of them
    for p in ps:
        img, _, info = MC.render(ms, cam, p)
        assert np.isfinite(img).all() and lively(img) and info["reached"][2] > 0
