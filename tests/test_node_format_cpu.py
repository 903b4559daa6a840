"""The f32 plane format of a sphere tree (rtw_host.h pack_nodes32, RTW_OPT_NODE_FORMAT), on the host alone.

The large-workgroup builds of the render kernel walk a copy of the tree whose planes are f32 and whose {near, far} pair a ray reads at a
per-ray offset.  The walk is the f16 walk only if (a) every plane is the f16 plane, widened, and (b) the offset rule hands a ray the
pair that min / max of the two plane distances would.  Both are checked here from the outside, through rtw_bvh_dump and
rtw_bvh_pack_nodes32."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests.test_bvh_builder_cpu import dump


def layout():
    lay = (C.c_uint32 * 4)()
    assert R.lib().rtw_bvh_pack_nodes32(None, 0, None, 0, lay) == 0
    return tuple(lay)          # dwords per node, dwords per (box, axis) group, +axis read offset in bytes, code per node index


def pack(nodes16):
    nd = layout()[0]
    n16 = np.ascontiguousarray(nodes16, np.uint16)
    out = np.zeros(len(n16) * nd, np.uint32)
    assert R.lib().rtw_bvh_pack_nodes32(n16.ctypes.data, len(n16), out.ctypes.data, out.size, None) == 0
    return out.reshape(len(n16), nd)


def hand_scene(n_small):
    """n_small small spheres and the ground (which the builder keeps outside the tree: 16 x the median radius and more)."""
    rng = np.random.default_rng(n_small)
    sp = [R.Sphere.with_albedo((0.0, -100.5, -1.0), 100.0, (0.5, 0.5, 0.5), R.SCATTER_M)]
    sp += [R.Sphere.with_albedo((float(1.1 * k - 0.55 * (n_small - 1)), float(rng.uniform(-0.2, 0.3)), float(-1.5 - 0.4 * (k % 3))), 0.3,
                                rng.uniform(0.2, 0.9, 3), (R.SCATTER_M, R.METALLIC_M, R.GLASS_M)[k % 3]) for k in range(n_small)]
    return R.Scene(sp)


SCENES = {"book1": lambda: R.Scene.generate(R.SCENE_C2), "2 spheres": lambda: hand_scene(2), "3 spheres": lambda: hand_scene(3),
          "5 spheres": lambda: hand_scene(5)}


def test_layout_is_the_documented_one():
    nd, ax, off, code = layout()
    assert (nd, ax, off, code) == (28, 4, 8, 14)     # six groups {hi, lo, lo, hi}, the child dword at 24 and 26, whole 16-byte rows; units of 8 bytes
    # the largest tree LDS can hold in f16 (512 nodes) stays below the DEAD code of the 16-bit stack entries
    assert 511 * code < 0x7FFE


@pytest.mark.parametrize("n_leaves", [2, 3, 6, 100, 481, 500, 512, 513])
def test_every_tree_with_f16_nodes_fits_two_large_workgroups(n_leaves):
    """The shim runs the f32 planes only where two 768-thread workgroups fit a CU's 160 KiB: nodes * 112 + (depth + 3 levels, at least 4)
    * 768 * 2 bytes, twice.  The builder caps the depth of a tree with f16 nodes so that nodes * 32 + levels * 512 fits a seventh of the
    160 KiB, and 3.5 x the one plus 3 x the other stays within half of it -- restated here for the deepest tree the builder may return at
    every size, from its own cap (bvh_depth_cap, through a scene of that many tree spheres).  And the rule itself (rtw_render_choice) answers
    f32 planes for each of them under the default options."""
    rng = np.random.default_rng(n_leaves)
    sp = [R.Sphere.with_albedo((0.0, -1000.0, 0.0), 1000.0, (0.5, 0.5, 0.5), R.SCATTER_M)]
    sp += [R.Sphere.with_albedo((float(rng.uniform(-8, 8)), 0.2, float(rng.uniform(-8, 8))), 0.2, (0.5, 0.5, 0.5), R.SCATTER_M) for _ in range(n_leaves)]
    d = dump(R.Scene(sp))
    assert len(d["nodes"]) == n_leaves - 1 and d["nodes16"].any()
    for depth in (d["depth"], d["cap"]):
        levels = max(depth + 3, 4)
        assert 2 * ((n_leaves - 1) * 28 * 4 + ((levels * 768 * 2 + 15) & ~15)) <= 160 * 1024, (n_leaves, depth)
        # RTW_OPT_NODE_FORMAT at its default throughout.  RTW_OPT_LDS_GEOM at its default (-1) sends a scene whose f16 nodes, 256-thread stack
        # and sphere geometry fit a sixth of the CU to the build that keeps all three in LDS (NODES == 2, f16), before the planes are asked
        # about; every other tree, and every tree with RTW_OPT_LDS_GEOM = 0, walks f32 planes.
        for lds_geom in (-1, 0):
            choice = R.render_choice(R.RtwRenderFacts(integrator=R.INTEGRATOR_GRADIENT, sampler=R.SAMPLER_ROW, depth=50),
                                     R.RtwTreeFacts(n_nodes=n_leaves - 1, depth=depth, n_spheres=len(sp), has_f16=1, has_planes=1), lds_geom=lds_geom)
            rides = lds_geom < 0 and (((n_leaves - 1) * 32 + 15) & ~15) + levels * 512 + len(sp) * 16 <= 160 * 1024 // 6
            want = ("render_bvh<0,2,1,0>", R.NODE_FORMAT_F16, 256) if rides else ("render_bvh<0,1,1,0>", R.NODE_FORMAT_F32, 768)
            assert (choice["build"], choice["node_format"], choice["block"]) == want, (n_leaves, depth, lds_geom, choice)
            if not rides:
                assert choice["lds_bytes"] == (n_leaves - 1) * 28 * 4 + ((levels * 768 * 2 + 15) & ~15)


@pytest.mark.parametrize("name", list(SCENES))
def test_planes_are_the_f16_planes_widened(name):
    d = dump(SCENES[name]())
    n16 = d["nodes16"]
    assert len(n16) == len(d["nodes"]) >= 1 and n16.any(), "the scene must have f16 nodes"
    nd, ax, off, code = layout()
    p = pack(n16)
    planes = n16[:, :12].view(np.float16).astype(np.float32).reshape(-1, 2, 3, 2)      # [node][box][axis]{lo, hi}, exact widening
    for c in range(2):
        for k in range(3):
            g = p[:, (c * 3 + k) * ax:(c * 3 + k + 1) * ax].view(np.float32)
            lo, hi = planes[:, c, k, 0], planes[:, c, k, 1]
            for j, w in enumerate([hi, lo, lo, hi]):
                assert np.array_equal(g[:, j].view(np.uint32), w.view(np.uint32)), (name, c, k, j)
    # children: a leaf keeps its code, an inner child index * 32 becomes index * code; found at both read offsets of the x group
    ch = n16[:, 12:14].astype(np.int16).astype(np.int64)
    want = np.where(ch >= 0, ch // 32 * code, ch) & 0xFFFF
    word = (want[:, 0] | (want[:, 1] << 16)).astype(np.uint32)
    assert np.array_equal(p[:, 6 * ax], word) and np.array_equal(p[:, 6 * ax + off // 4], word)
    assert (want[ch >= 0] < 0x7FFE).all() and (want[ch < 0] > 0x7FFF).all()


@pytest.mark.parametrize("inv", [2.5, -2.5, 1e20, -1e20, float(np.float32(1.0) / np.float32(1e-30)), float(np.float32(1.0) / np.float32(-1e-30)),
                                 float(np.copysign(np.float32(1e20), np.float32(0.0))), float(np.copysign(np.float32(1e20), np.float32(-0.0)))])
def test_offset_rule_gives_near_and_far(inv):
    """The pair a ray reads -- at the +axis offset when the sign bit of 1/d is clear, at 0 when it is set (the rule the f16 walk's byte
    permute follows; 1/d of a zero component is +-1e20 by the sign of the component, so -0.0 reads at 0) -- is {near, far} by min / max."""
    nd, ax, off, code = layout()
    d = dump(SCENES["book1"]())
    p = pack(d["nodes16"])
    f = np.float32
    inv = f(inv)
    o = f(0.37)
    sign = (np.array([inv]).view(np.uint32)[0] >> 31) & 1
    at = 0 if sign else off // 4
    for g0 in range(0, 6 * ax, ax):
        pair = p[:, g0 + at:g0 + at + 2].view(np.float32)
        planes = p[:, g0:g0 + 2].view(np.float32)                      # {hi, lo}
        t = (planes - o) * inv
        assert np.array_equal((pair[:, 0] - o) * inv, t.min(axis=1)) and np.array_equal((pair[:, 1] - o) * inv, t.max(axis=1))
