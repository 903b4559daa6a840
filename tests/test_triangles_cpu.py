"""Rust2 triangles on the host (no GPU): Triangle::new and get_hit (Rust2/src/objects/triangle.rs:28-124) against an independent numpy f32
restatement, the reference's triangle_test triangle by hand, the tree's self-check, argument checks."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R

f32 = np.float32


# ---- numpy restatement of triangle.rs, one f32 rounding per written operation ----------------------------------------------------------
def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def tri_new(o, u, v):
    """Triangle::new (:28-50): (normal, d, w)."""
    o, u, v = (np.asarray(x, f32) for x in (o, u, v))
    with np.errstate(all="ignore"):
        n = cross(u, v)
        ln = np.sqrt(dot(n, n))
        normal = n / ln[..., None]
        d = dot(normal, o)
        w = n / dot(n, n)[..., None]
    return normal, d, w


def tri_hits_np(O, U, V, rays, mint, maxt):
    """The closest triangle of the list per ray (the group rule of rtw.h), get_hit (:95-124) as written."""
    O, U, V = (np.asarray(x, f32).reshape(-1, 3) for x in (O, U, V))
    N, D, W = tri_new(O, U, V)
    r = np.asarray(rays, f32).reshape(-1, 6)
    ro, rd = r[:, None, 0:3], r[:, None, 3:6]
    mint, maxt = f32(mint), f32(maxt)
    with np.errstate(all="ignore"):
        den = dot(N[None], rd)
        t = (D[None] - dot(N[None], ro)) / den
        ok = ~(np.abs(den) <= f32(1e-8)) & ~((t < mint) | (t > maxt))
        p = ro + rd * t[..., None]
        planar = p - O[None]
        alfa = dot(W[None], cross(planar, np.broadcast_to(V[None], planar.shape)))
        beta = dot(W[None], cross(np.broadcast_to(U[None], planar.shape), planar))
        ok &= ~((alfa < 0) | (beta < 0) | (alfa + beta > 1))
    best_t = np.full(len(r), np.inf, f32)
    best_i = np.full(len(r), -1, np.int32)
    for k in range(len(O)):                      # list order, a later one only when strictly closer
        tk = t[:, k]
        take = ok[:, k] & ((best_i < 0) | (best_t > tk))
        best_t = np.where(take, tk, best_t)
        best_i = np.where(take, k, best_i)
    return best_t, best_i


def pods(O, U, V):
    O, U, V = (np.asarray(x, f32).reshape(-1, 3) for x in (O, U, V))
    return R.TriangleArray(O, U, V)


def same(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) or np.array_equal(a, b, equal_nan=True) and np.array_equal(np.isnan(a), np.isnan(b))


def random_mesh(rng, n, scale=4.0, size=0.6):
    O = rng.uniform(-scale, scale, (n, 3)).astype(f32)
    U = rng.uniform(-size, size, (n, 3)).astype(f32)
    V = rng.uniform(-size, size, (n, 3)).astype(f32)
    return O, U, V


# ---- the reference's triangle_test scene (Rust2/src/objects/triangle.rs:162-200) as a numpy known answer ----------------------------
def reference_triangle_test():
    """One grey Lambert triangle (ConstColorTexture(WHITE * 0.5, BLACK)) on a 0.6 background, Rust2's camera and fixed-centre sampler,
    400 x 300 x 25, depth 2.  The numpy answer: the camera rays of the fixed-centre sampler (Rust2/src/viewport.rs:92-104), coverage by
    the triangle, 0.6 * 0.5 or 0.6 per sample, added in sample order and divided by 25.
    Returns (scene, camera, params, want [H][W] f32, hit [H * W * S] triangle index per camera ray)."""
    W, H, S = 400, 300, 25
    tri = R.Triangle.new((1, -1, 3), (-1, 2, 0), (-2, 1, 0), R.SCATTER_M, (0.5, 0.5, 0.5), (0.0, 0.0, 0.0))
    scene = R.Scene([], background=(0.6, 0.6, 0.6), triangles=[tri])
    cam = R.camera2_new(f32(W) / f32(H), (0, 0, 0), (0, 1, 0), (0, 0, 1), 50.0, 0.0)
    p = R.RtwParams()
    p.width, p.height, p.samples, p.depth, p.gamma = W, H, S, 2, 1.0
    p.mint, p.maxt = 0.0001, 10000.0
    p.integrator, p.sampler, p.flags, p.seed = R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, 0, 77
    s_root = 5
    i = np.arange(W, dtype=f32)[None, :, None]
    j = np.arange(H, dtype=f32)[:, None, None]
    s = np.arange(S)
    kx, ly = (s // s_root).astype(f32), (s % s_root).astype(f32)
    jx = (i + (kx + f32(0.5)) / f32(s_root)) / f32(W)
    jy = (j + (ly + f32(0.5)) / f32(s_root)) / f32(H)
    p00, du, dv = (np.array(x, f32) for x in (cam.pixel00, cam.delta_u, cam.delta_v))
    d = (p00 + du * jx[..., None]) + dv * jy[..., None]
    o = np.broadcast_to(np.array(cam.origin, f32), d.shape)
    rays = np.concatenate([o, d], -1).reshape(-1, 6)
    _, hit = tri_hits_np([tri.pod.origin], [tri.pod.u], [tri.pod.v], rays, 0.0001, 10000.0)
    val = np.where(hit.reshape(H, W, S) >= 0, f32(0.6) * f32(0.5), f32(0.6)).astype(f32)
    acc = np.zeros((H, W), f32)
    for q in range(S):
        acc = acc + val[:, :, q]
    return scene, cam, p, acc / f32(S), hit


# ---- Triangle::new ---------------------------------------------------------------------------------------------------------------
def test_triangle_new_matches_restatement_bitwise():
    rng = np.random.default_rng(1)
    O, U, V = random_mesh(rng, 300, 100.0, 5.0)
    N, D, W = tri_new(O, U, V)
    for i in range(len(O)):
        t = R.Triangle.new(O[i], U[i], V[i], mat=(0.25, 0.0, 1.5), color=(0.1, 0.2, 0.3), emitted=(1, 2, 3), tex_index=-1).pod
        assert same(list(t.normal), N[i]) and same([t.d], [D[i]]) and same(list(t.w), W[i]), i
        assert list(t.tex_color) == [f32(0.1), f32(0.2), f32(0.3)] and list(t.emitted) == [1, 2, 3] and t.tex == -1
        assert (t.metallicness, t.opacity, t.ir) == (0.25, 0.0, 1.5)


def test_reference_triangle_test_known_answers():
    # Rust2's LEFT = +x, RIGHT = -x, UP = +y, FORWARD = +z: origin LEFT + DOWN + 3 FORWARD, u = 2 UP + RIGHT, v = 2 RIGHT + UP
    t = R.Triangle.new((1, -1, 3), (-1, 2, 0), (-2, 1, 0)).pod
    assert list(t.normal) == [0.0, 0.0, 1.0] and t.d == 3.0                     # n = (0, 0, 3): unit (0, 0, 1), d = 3
    assert list(t.w) == [0.0, 0.0, float(f32(1) / f32(3))]                       # w = n / 9
    # a camera ray along +z from the origin: t = 3 at the plane z = 3; (0,0,3) - origin = (-1, 1, 0) = alfa u + beta v with alfa = beta = 1/3
    rays = np.array([[0, 0, 0, 0, 0, 1],        # inside
                     [0, 0, 0, 1, -1, 3],       # straight at the origin vertex: alfa = beta = 0 (inside, closed)
                     [0, 0, 0, 0, 0, -1],       # away: t = -3 < mint
                     [0, 0, 0, 1, 0, 0],        # parallel: |n.d| = 0
                     [0, 0, 0, 3, 3, 3]],       # through (3, 3, 3): outside
                    f32)
    t_out, idx = R.triangle_hits([R.Triangle(t)], rays, 1e-4, 1e4)
    assert list(idx) == [0, 0, -1, -1, -1]
    assert t_out[0] == 3.0 and t_out[1] == 1.0 and np.isinf(t_out[2:]).all()


def test_degenerate_triangle_reports_nan_hit():
    tri = R.Triangle.new((0, 0, 0), (1, 1, 1), (2, 2, 2)).pod           # u x v == 0
    assert all(np.isnan(list(tri.normal))) and np.isnan(tri.d)
    rays = np.array([[5, -3, 2, 0.3, 0.1, -1], [0, 0, 0, 1, 0, 0]], f32)
    t_out, idx = R.triangle_hits([R.Triangle(tri), R.Triangle.new((0, 0, -1), (1, 0, 0), (0, 1, 0)).pod], rays, 1e-3, 1e4)
    assert list(idx) == [0, 0] and np.isnan(t_out).all()                # the NaN hit blocks every later candidate, as in the reference


# ---- the host list walk against the restatement ----------------------------------------------------------------------------------
def adversarial_rays(rng, O, U, V, n):
    """Rays at vertices and shared edges, grazing the plane, at t == mint / maxt, with huge or NaN coordinates."""
    k = rng.integers(0, len(O), n)
    o, u, v = O[k], U[k], V[k]
    choice = rng.integers(0, 6, n)
    a = rng.uniform(0, 1, n).astype(f32)
    target = np.where((choice == 0)[:, None], o, np.where((choice == 1)[:, None], o + u, np.where((choice == 2)[:, None], o + v,
                      o + u * a[:, None] + (v - u) * (1 - a[:, None]) * f32(0))))
    target = np.where((choice == 3)[:, None], o + u * a[:, None], target)            # an edge from the origin vertex
    target = np.where((choice == 4)[:, None], (o + u) + (v - u) * a[:, None], target)  # the edge opposite it
    src = rng.uniform(-8, 8, (n, 3)).astype(f32)
    d = target - src
    rays = np.concatenate([src, d], 1).astype(f32)
    # grazing: direction nearly in the plane, |n.d| around 1e-8
    N, _, _ = tri_new(o, u, v)
    g = rng.random(n) < 0.15
    tangent = u / np.linalg.norm(u, axis=1, keepdims=True).astype(f32)
    eps = rng.choice(np.array([0.5e-8, 1e-8, 1.0000001e-8, 2e-8, 0.0], f32), n)
    rays[g, 3:6] = (tangent + N * eps[:, None])[g]
    rays[g, 0:3] = (o + u * f32(0.3) + v * f32(0.3) - tangent * f32(2))[g]
    # huge and NaN coordinates
    h = rng.random(n) < 0.05
    rays[h, 0] = f32(3e38)
    nn = rng.random(n) < 0.03
    rays[nn, 4] = np.nan
    return rays


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_host_hits_match_restatement(seed):
    rng = np.random.default_rng(seed)
    O, U, V = random_mesh(rng, 60)
    rays = np.concatenate([np.concatenate([rng.uniform(-8, 8, (3000, 3)), rng.normal(size=(3000, 3))], 1).astype(f32),
                           adversarial_rays(rng, O, U, V, 3000)])
    t_ref, i_ref = tri_hits_np(O, U, V, rays, 1e-3, 1e4)
    t, i = R.triangle_hits(pods(O, U, V), rays, 1e-3, 1e4)
    assert np.array_equal(i, i_ref)
    assert same(t, t_ref)
    assert (i >= 0).sum() > 1000


def test_host_hits_at_mint_and_maxt():
    O, U, V = np.array([[-1, -1, 2]], f32), np.array([[4, 0, 0]], f32), np.array([[0, 4, 0]], f32)
    rays = np.array([[0, 0, 0, 0, 0, 1], [0, 0, 1, 0, 0, 1], [0, 0, 0, 0, 0, 0.5]], f32)
    for mint, maxt in ((2.0, 4.0), (1.0, 2.0), (2.0000002, 4.0), (0.0, 1.9999999), (4.0, 4.0)):
        t_ref, i_ref = tri_hits_np(O, U, V, rays, mint, maxt)
        t, i = R.triangle_hits(pods(O, U, V), rays, mint, maxt)
        assert np.array_equal(i, i_ref) and same(t, t_ref), (mint, maxt)
    t, i = R.triangle_hits(pods(O, U, V), rays[:1], 2.0, 2.0)
    assert i[0] == 0 and t[0] == 2.0                                   # t == mint == maxt is inside the closed range


def test_host_hits_nan_and_coincident():
    O = np.array([[-1, -1, 2], [-1, -1, 2], [-1, -1, 1], [np.nan, 0, 0]], f32)
    U = np.array([[4, 0, 0], [4, 0, 0], [4, 0, 0], [1, 0, 0]], f32)
    V = np.array([[0, 4, 0], [0, 4, 0], [0, 4, 0], [0, 1, 0]], f32)
    rays = np.array([[0, 0, 0, 0, 0, 1], [0, 0, 5, 0, 0, -1], [0, 0, 0, np.nan, 0, 1], [-5, 0, 0, 1, 0, 0.1]], f32)
    for mint, maxt in ((1e-3, 1e4), (np.nan, 1e4), (1e-3, np.inf)):
        t_ref, i_ref = tri_hits_np(O, U, V, rays, mint, maxt)
        t, i = R.triangle_hits(pods(O, U, V), rays, mint, maxt)
        assert np.array_equal(i, i_ref) and same(t, t_ref), (mint, maxt, i, i_ref)


# ---- the tree's self-check -------------------------------------------------------------------------------------------------------
def grid_mesh(n_side, rng=None, height=0.0):
    xs = np.linspace(-10, 10, n_side + 1, dtype=f32)
    X, Z = np.meshgrid(xs, xs)
    Y = np.zeros_like(X) if rng is None else (rng.random(X.shape) * height).astype(f32)
    vtx = np.stack([X, Y, Z], -1).reshape(-1, 3)
    i = np.arange(n_side)
    a = (i[:, None] * (n_side + 1) + i[None, :]).reshape(-1)
    faces = np.concatenate([np.stack([a, a + 1, a + n_side + 1], 1), np.stack([a + 1, a + n_side + 2, a + n_side + 1], 1)])
    return vtx, faces


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 17, 1000, 20000])
def test_bvh_validate_random(n):
    rng = np.random.default_rng(n)
    rc, n_nodes, depth, walk = R.triangle_bvh_validate(pods(*random_mesh(rng, n)))
    assert rc == 0 and walk == 0 and n_nodes >= 1 and depth <= 64


def test_bvh_validate_terrain_200k():
    vtx, faces = grid_mesh(317, np.random.default_rng(5), 1.5)           # 2 * 317^2 = 200978 triangles
    m = R.Triangle.from_mesh(vtx, faces)
    assert len(m) > 200000
    rc, n_nodes, depth, walk = R.triangle_bvh_validate(m)
    assert rc == 0 and walk == 0 and depth <= 64 and n_nodes < len(m)


def test_bvh_validate_slivers_and_coincident():
    rng = np.random.default_rng(9)
    O, U, V = random_mesh(rng, 500)
    O[100:200] = O[100]; U[100:200] = U[100]; V[100:200] = V[100]          # coincident
    V[300:400] = U[300:400] * f32(1.0) + f32(0.01) * V[300:400]            # slivers (kappa up to ~100s)
    rc, _, _, walk = R.triangle_bvh_validate(pods(O, U, V))
    assert rc == 0
    V[450] = U[450] * f32(2)                                              # degenerate: NaN derived fields -> the list walk
    rc, _, _, walk = R.triangle_bvh_validate(pods(O, U, V))
    assert rc == 0 and walk == 1


@pytest.mark.parametrize("what", ["nan", "far", "sliver"])
def test_bvh_validate_reports_the_list_walk_conditions(what):
    O, U, V = random_mesh(np.random.default_rng(3), 50)
    if what == "nan":
        O[7, 1] = np.nan
    elif what == "far":
        O[7] = f32(1e30)                                                   # a coordinate beyond 2^40
    else:
        V[7] = U[7] + U[7] * f32(1e-4)                                     # max(|u|,|v|)^2 / |u x v| > 256
    rc, _, _, walk = R.triangle_bvh_validate(pods(O, U, V))
    assert rc == 0 and walk == 1


def test_from_mesh_fields():
    vtx = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1.1, 1.3, 0.7]], f32)
    m = R.Triangle.from_mesh(vtx, [[0, 1, 2], [1, 3, 2]], mat=R.METALLIC_M, color=(0.5, 0.5, 0.5))
    t = m[1].pod
    assert list(t.origin) == list(vtx[1]) and list(t.u) == list(vtx[3] - vtx[1]) and list(t.v) == list(vtx[2] - vtx[1])
    assert t.metallicness == 1.0 and t.tex == -1 and list(t.tex_color) == [0.5] * 3
    with pytest.raises(ValueError):
        R.Triangle.from_mesh(vtx, [[0, 1, 4]])


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    L = R.lib()
    fp = C.POINTER(C.c_float)
    o = (C.c_float * 3)(0, 0, 0)
    out = R.RtwTriangle()
    assert L.rtw_triangle_new(None, o, o, None, None, o, -1, C.byref(out)) == -1
    assert L.rtw_triangle_new(o, o, o, None, None, None, -1, C.byref(out)) == -1
    assert L.rtw_triangle_new(o, o, o, None, None, o, -2, C.byref(out)) == -1
    assert L.rtw_triangle_new(o, o, o, None, None, o, -1, None) == -1
    arr = (R.RtwTriangle * 1)(out)
    rays = (C.c_float * 6)()
    t = (C.c_float * 1)()
    i = (C.c_int32 * 1)()
    assert L.rtw_triangle_hits(arr, 1, rays, 0, 0.0, 1.0, t, i) == -1
    assert L.rtw_triangle_hits(None, 1, rays, 1, 0.0, 1.0, t, i) == -1
    assert L.rtw_triangle_hits(arr, 1, None, 1, 0.0, 1.0, t, i) == -1
    assert L.rtw_triangle_hits(arr, 1, rays, 1, 0.0, 1.0, None, i) == -1
    assert L.rtw_triangle_hits(None, 0, rays, 1, 0.0, 1.0, t, i) == 0 and i[0] == -1   # no triangles: every ray misses
    assert L.rtw_triangle_bvh_validate(None, 0, None, None, None) == -1
    assert L.rtw_triangle_bvh_validate(None, 3, None, None, None) == -1
    assert L.rtw_ctx_set_triangles(None, arr, 1) == -1
    assert L.rtw_mgpu_set_triangles(None, arr, 1) == -1
    assert L.rtw_ctx_triangle_hits(None, rays, 1, 0.0, 1.0, 0, t, i, None) == -1
    with pytest.raises(ValueError):
        R.triangle_hits(arr, np.zeros((0, 6), f32), 0.0, 1.0)
    assert fp  # (pointer type used by the argtypes above)
