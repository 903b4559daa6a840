"""Rust2's quaternion-rotated instances, the host side (no GPU): the host functions rtw_quat_* against the restatement of
tests/quat_common.py bit for bit, known answers of the reference's rotation_test and nor_rot, every status of
rtw_instance_rotations_validate, and the sanity of the fixture tests/golden/rust2_rotation_scene.json."""
import numpy as np

import rtw_amd as R
from tests import quat_common as Q

F = np.float32
E_INVALID = -1


def same_bits(a, b):
    """Bit-equal, or NaN in both (a NaN's payload is not part of the contract)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def test_rotate_equals_the_restatement_on_random_pairs():
    rng = np.random.default_rng(11)
    q = rng.normal(size=(10000, 4)).astype(F) * np.exp2(rng.integers(-6, 7, size=(10000, 1))).astype(F)
    v = rng.normal(size=(10000, 3)).astype(F) * np.exp2(rng.integers(-10, 11, size=(10000, 1))).astype(F)
    ref = Q.rotate(q, v)
    got = np.array([R.quat_rotate(q[i], v[i]) for i in range(len(q))], F)
    bad = ~((Q.bits(got) == Q.bits(ref)) | (np.isnan(got) & np.isnan(ref)))
    print(f"quat_rotate: {int(bad.sum())} of {bad.size} values differ from the restatement")
    assert not bad.any()
    # the rotation is one: lengths are kept to rounding (|v'| / |v| - 1 within a few ulp of the 30-odd operations)
    l0, l1 = np.linalg.norm(v.astype(np.float64), axis=1), np.linalg.norm(got.astype(np.float64), axis=1)
    assert np.max(np.abs(l1 / l0 - 1.0)) < 64 * 2.0 ** -24


def test_rotate_edge_values():
    """The identity, q and -q, unnormalised q of length 1e-3 and 1e3, and v with a -0, an inf and a NaN component: the restatement's bits,
    signed zeros included."""
    g = Q.golden()
    q0 = Q.f32(g["quaternion_wxyz"])
    qs = [Q.f32([1, 0, 0, 0]), q0, -q0, (q0 * F(1e-3)).astype(F), (q0 * F(1e3)).astype(F), Q.f32([0.3, -0.5, 0.7, 0.1]), Q.f32([0, 0, 1, 0]),
          Q.f32([-0.0, 0.0, -0.0, 2.0])]
    vs = [Q.f32([0, 0, 1]), Q.f32([1, 2, 3]), Q.f32([-0.0, 1.0, 0.0]), Q.f32([0.0, -0.0, -0.0]), Q.f32([-0.0, -0.0, -0.0]), Q.f32([0, 0, 0]),
          Q.f32([np.inf, 1.0, -2.0]), Q.f32([1.0, -np.inf, 0.0]), Q.f32([np.nan, 1.0, 2.0]), Q.f32([1.0, 2.0, np.nan]), Q.f32([1e30, -1e30, 1e-30])]
    n = 0
    for q in qs:
        for v in vs:
            ref, got = Q.rotate(q, v), R.quat_rotate(q, v)
            assert same_bits(got, ref), (q, v, got, ref)
            n += 1
    assert n == len(qs) * len(vs)
    # q and -q are the same rotation, and so is any positive multiple up to the rounding of its normalisation
    assert same_bits(R.quat_rotate(q0, vs[1]), R.quat_rotate(-q0, vs[1]))
    for s in (1e-3, 1e3):
        assert np.allclose(R.quat_rotate((q0 * F(s)).astype(F), vs[1]), R.quat_rotate(q0, vs[1]), rtol=0, atol=1e-5)


def test_mul_from_axis_from_euler_equal_the_restatement():
    rng = np.random.default_rng(5)
    for _ in range(500):
        a, b = rng.normal(size=4).astype(F), rng.normal(size=4).astype(F)
        assert same_bits(R.quat_mul(a, b), Q.hamilton(a, b))
        angle, axis = F(rng.uniform(-7, 7)), (rng.normal(size=3) * 3).astype(F)
        assert same_bits(R.quat_from_axis(angle, axis), Q.from_axis(angle, axis)), (angle, axis)
        e = rng.uniform(-4, 4, size=3).astype(F)
        assert same_bits(R.quat_from_euler(e), Q.from_euler(e)), e
    assert same_bits(R.quat_mul([1, 0, 0, 0], [0.5, 1, 2, 3]), [0.5, 1, 2, 3])
    # a zero axis is not guarded (Vec3::unit divides by 0): NaN vector part, as in the reference
    assert np.isnan(R.quat_from_axis(1.0, [0, 0, 0])[1:]).all()


def test_known_answers():
    g = Q.golden()
    q = R.quat_from_axis(F(np.pi) / F(4.0), [0, 1, 0])            # rotation_test: Quaternion::new_from_axis(PI / 4., Vec3::UP)
    assert same_bits(q, g["quaternion_wxyz"]) and same_bits(q, Q.from_axis(g["quaternion_axis_angle"]["angle"], g["quaternion_axis_angle"]["axis"]))
    assert abs(float(q[0]) - np.cos(np.pi / 8)) < 1e-7 and abs(float(q[2]) - np.sin(np.pi / 8)) < 1e-7 and q[1] == 0 and q[3] == 0
    # Instance::rotate on a fresh instance: ZERO_ROTATION.hamilton(q) is q
    assert same_bits(R.quat_mul([1, 0, 0, 0], q), q)
    # a quarter of a turn about UP takes FORWARD half way to +x: (sin 45, 0, cos 45)
    r = R.quat_rotate(q, [0, 0, 1])
    assert np.allclose(r, [np.sqrt(0.5), 0, np.sqrt(0.5)], atol=2e-7), r
    assert same_bits(r, Q.rotate(q, [0, 0, 1]))
    # nor_rot (quaternions.rs:199-210): the identity on FORWARD gives FORWARD, and the half product is not short
    assert same_bits(R.quat_rotate([1, 0, 0, 0], [0, 0, 1]), [0, 0, 1])
    half = R.quat_mul([1, 0, 0, 0], [0, 0, 0, 1])
    assert float(half[1] ** 2 + half[2] ** 2 + half[3] ** 2) > 1e-10
    assert same_bits(R.quat_mul(half, [1, -0.0, -0.0, -0.0])[1:], [0, 0, 1])


def test_instance_rotations_validate():
    g = Q.golden()
    qs = Q.fixture_scene(g)
    q = [g["quaternion_wxyz"]]
    V = R.instance_rotations_validate
    assert V(qs.scene, q) == 0
    assert V(qs.scene, None) == 0                                  # NULL / 0 clears
    assert V(qs.scene, [[1, 0, 0, 0]]) == 0 and V(qs.scene, [[0, 0, 5e3, 0]]) == 0 and V(qs.scene, [[1e-3, 0, 0, 0]]) == 0
    assert V(qs.scene, q + q) == E_INVALID                         # count mismatch
    two = Q.fixture_scene(g, extra_instances=[Q.box_instance(g)])
    assert V(two.scene, q) == E_INVALID and V(two.scene, q + q) == 0
    for bad in ([np.nan, 0, 0, 1], [1, np.inf, 0, 0], [1, 0, -np.inf, 0], [0, 0, 0, np.nan]):
        assert V(qs.scene, [bad]) == E_INVALID, bad                # a component that is not finite
    assert V(qs.scene, [[0, 0, 0, 0]]) == E_INVALID and V(qs.scene, [[-0.0, 0, 0, 0]]) == E_INVALID        # len 0
    assert V(qs.scene, [[1e-30, 0, 0, 0]]) == E_INVALID            # w * w underflows: len 0
    assert V(qs.scene, [[3e38, 3e38, 0, 0]]) == E_INVALID and V(qs.scene, [[2e19, 0, 0, 0]]) == E_INVALID  # len overflows
    # a non-zero Euler rotation on the same instance, and a constant-density instance
    box = R.Instance.new_box([-1, -1, -1], [1, 1, 1], [0.6, 0.6, 0.6], (0.0, 0.0, 1.0))
    box.rotate([0.0, 0.1, 0.0])
    assert V(R.Scene([], instances=[box]), q) == E_INVALID
    box = R.Instance.new_box([-1, -1, -1], [1, 1, 1], [0.6, 0.6, 0.6], (0.0, 0.0, 1.0))
    assert V(R.Scene([], instances=[box]), q) == 0
    box.const_density(0.5)
    assert V(R.Scene([], instances=[box]), q) == E_INVALID
    assert V(R.Scene([]), None) == 0 and V(R.Scene([]), q) == E_INVALID


def test_fixture_is_the_reference_scene_and_its_depth_map_is_sane():
    """The fixture's numbers against what rotation_test writes, and the condition that shows the camera sees the turned box: in the restated
    48 x 48 depth map between 10 % and 90 % of the pixels hit the box and at least two different quads are hit."""
    g = Q.golden()
    assert g["translation"] == [-1.0, 0.0, 5.0] and g["mint"] == 1e-4 and g["maxt"] == 1e4            # FORWARD * 5 + RIGHT (RIGHT is -x)
    assert g["camera"] == {"aspect": 1.0, "origin": [0, 0, 0], "vup": [0, 1, 0], "direction": [0, 0, 1], "vfov": 50.0, "lens_radius": 0.0}
    assert g["background"] == [0.6] * 3 and g["color"] == [0.6] * 3 and g["gamma"] == 1.0 and g["depth"] == 2 and g["samples"] == 25
    # Instance::new_box(-1, +1): the library's box constructor lays the same six quads down in the same order
    lib_box = R.Instance.new_box([-1, -1, -1], [1, 1, 1], g["color"], (0.0, 0.0, 1.0))
    assert len(g["box_quads"]) == 6
    for a, b in zip(g["box_quads"], lib_box.quads):
        assert same_bits(a["origin"], list(b.origin)) and same_bits(a["u"], list(b.u)) and same_bits(a["v"], list(b.v))
    qs = Q.fixture_scene(g)
    o, d = Q.depth_rays(Q.camera(g, 48, 48), 48, 48)
    h = qs.closest(o, d)
    frac = h["found"].mean()
    members = sorted(set((~h["member"][h["found"]]).tolist()))
    print(f"fixture depth map 48 x 48: {100 * frac:.1f} % of the pixels hit the box, quads hit: {members}")
    assert 0.10 <= frac <= 0.90
    assert len(members) >= 2
    assert set(h["idx"][h["found"]].tolist()) == {0}
    # the hits are on the turned box: within sqrt(3) of its centre, normals of unit length
    c = np.array(g["translation"])
    assert np.all(np.linalg.norm(h["point"][h["found"]] - c, axis=1) <= np.sqrt(3) + 1e-5)
    assert np.allclose(np.linalg.norm(h["normal"][h["found"]], axis=1), 1.0, atol=1e-6)
    # Euler rotation 0 in place of the quaternion is another picture: the fixture does test the rotation
    flat = Q.QuatScene(instances=[Q.box_instance(g, quat=[1, 0, 0, 0])], background=g["background"], mint=g["mint"], maxt=g["maxt"])
    assert (flat.closest(o, d)["found"] != h["found"]).any()


def test_restated_closest_matches_the_oracle_without_rotation():
    """With the identity quaternion the restated instance walk is the Euler walk with rotation 0 -- up to the identity rotation's own
    arithmetic, which is exact on these operands: the restated t / index of the unrotated box scene equal the frozen oracle's closest hit."""
    from tests import lights_common as LC
    g = Q.golden()
    flat = Q.QuatScene(spheres=[{"origin": [1.5, 0.2, 4.0], "radius": 0.5, "material": "lambertian", "color": [0.5] * 3, "emitted": [0] * 3}],
                       instances=[Q.box_instance(g, quat=[1, 0, 0, 0])], background=g["background"], mint=g["mint"], maxt=g["maxt"])
    cam = Q.camera(g, 16, 16)
    o, d = Q.depth_rays(cam, 16, 16)
    h = flat.closest(o, d)
    p1 = flat.params(16, 16, R.INTEGRATOR_RUST2, 1)
    n_hit = 0
    for k in range(len(o)):
        r = LC.closest(flat, o[k], d[k], p1, k)
        assert (r is not None) == bool(h["found"][k]), k
        if r is not None:
            assert same_bits(r[1], h["t"][k]) and same_bits(r[2], h["point"][k]) and same_bits(r[3], h["normal"][k]), k
            n_hit += 1
    assert n_hit > 20
