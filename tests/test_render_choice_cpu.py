"""Which build a render launches and how its dynamic LDS is laid out (rtw_render_choice, include/rtw.h), on the host alone.

The render forms plain facts -- what the request needs, what the sphere tree allows -- and asks three functions once each; rtw_render_choice
asks the same three.  Here: every compiled build is reachable from some facts and nothing else is, a few known rows, and the LDS layout
against a restatement of the rule in Python, written from the shim's earlier in-line code and independent of the library's."""
import itertools
import math

import pytest

import rtw_amd as R
from tests import builds_common as B
from tests.test_bvh_builder_cpu import LDS_GEOM_MAX, STACK, dump, expected_cap

CU_LDS = 160 * 1024
BLOCK, BLOCK_LARGE = 256, 768
# the builds whose workgroup is 768 threads and whose tree is f32 planes (tests/test_gpu_large_block_budget.py)
LARGE_BUILDS = {"render_bvh<0,1,1,0>", "render_bvh<0,1,2,0>", "render_bvh<0,1,3,0>"}
COMMON = dict(integrator=R.INTEGRATOR_GRADIENT, sampler=R.SAMPLER_ROW, depth=50)          # the bench configuration: SPEC 1, 768 threads when static
DEMO = dict(integrator=R.INTEGRATOR_BG_COLOR, sampler=R.SAMPLER_ROW, depth=50)            # presentation_image's: SPEC 4, 256 threads


def facts(**kw):
    return R.RtwRenderFacts(**kw)


def tree(n_nodes, depth, n_spheres, f16=True):
    return R.RtwTreeFacts(n_nodes=n_nodes, depth=depth, n_spheres=n_spheres, has_f16=int(f16), has_planes=int(f16))


# ---- reachability ----------------------------------------------------------------------------------------------------------------------
def test_the_reachable_builds_are_the_compiled_ones():
    """The full cross product of request facts, with a sphere moving or none, over the list walk and the three NODES outcomes of a tree
    (no f16 nodes: 0; f16 nodes and RTW_OPT_LDS_GEOM = 0: 1; = 1: 2 where the request has such a build): every choice is a compiled build,
    and every compiled build is chosen."""
    small = {0: tree(5, 3, 7, f16=False), 1: tree(5, 3, 7), 2: tree(5, 3, 7)}
    f = facts()
    seen = set()
    flag_sets = [a | b | c for a in (0, R.FLAG_CPP_DIELECTRIC, R.FLAG_CPP_DIFFUSE) for b in (0, R.FLAG_CHUNK_SUMS) for c in (0, R.FLAG_MIXED_MATERIAL)]
    for f.integrator, f.sampler, f.depth, f.flags, f.has_textures in itertools.product(range(7), range(4), (0, 1), flag_sets, (0, 1)):
        for f.n_quads, f.n_instances, f.noise, f.n_triangles, f.rotations, f.placements in itertools.product((0, 1), repeat=6):
            for moving in (False, True):
                seen.add(R.render_choice(f, small[0], moving=moving, accel=R.ACCEL_BRUTE)["build"])
                for nodes, lds_geom in ((0, -1), (1, 0), (2, 1)):
                    seen.add(R.render_choice(f, small[nodes], lds_geom=lds_geom, moving=moving)["build"])
    compiled = B.library_builds()
    assert len(compiled) == 146
    assert seen == compiled, (sorted(seen - compiled), sorted(compiled - seen))


def test_known_rows():
    d = dump(R.Scene.generate(R.SCENE_C2))                       # Book-1: 485 spheres, the bench scene
    t = tree(len(d["nodes"]), d["depth"], 485)
    assert d["nodes16"].any() and len(d["nodes"]) == 485 - len(d["big"]) - 1
    bench = R.render_choice(facts(**COMMON), t)
    assert (bench["build"], bench["node_format"], bench["block"]) == ("render_bvh<0,1,1,0>", R.NODE_FORMAT_F32, BLOCK_LARGE)
    assert bench["lds_stack_off"] == len(d["nodes"]) * 112 and bench["lds_geom_off"] == 0 and 2 * bench["lds_bytes"] <= CU_LDS
    for lds_geom in (-1, 0, 1):                                  # RTW_OPT_NODE_FORMAT = 1: the f16 walk with the geometry in LDS, whatever RTW_OPT_LDS_GEOM says
        f16 = R.render_choice(facts(**COMMON), t, lds_geom=lds_geom, node_format=1)
        assert (f16["build"], f16["node_format"], f16["block"]) == ("render_bvh<0,2,1,0>", R.NODE_FORMAT_F16, BLOCK), (lds_geom, f16)
        assert f16["lds_bytes"] == f16["lds_geom_off"] + 485 * 16
    glob = R.render_choice(facts(flags=R.FLAG_GLOBAL_NODES, **COMMON), t)
    assert (glob["build"], glob["node_format"], glob["block"]) == ("render_bvh<0,0,1,0>", R.NODE_FORMAT_NONE, BLOCK)
    assert glob["lds_stack_off"] == 0 and glob["lds_bytes"] == max(d["depth"] + 3, 4) * BLOCK * 4
    walk = R.render_choice(facts(**COMMON), t, accel=R.ACCEL_BRUTE)
    assert walk == dict(build="render_brute<0,1,0>", node_format=0, block=BLOCK, lds_stack_off=0, lds_geom_off=0, lds_tri_off=0, lds_bytes=0)


def test_arguments_out_of_range_are_refused():
    f, t = facts(**COMMON), tree(5, 3, 7)
    for kw in (dict(accel=2), dict(lds_geom=-2), dict(lds_geom=2), dict(node_format=3)):
        with pytest.raises(R.RtwError) as e:
            R.render_choice(f, t, **kw)
        assert e.value.status == -1, kw
    assert R.lib().rtw_render_choice(None, None, -1, 0, 0, 1, None) == -1


# ---- layout ----------------------------------------------------------------------------------------------------------------------------
def align16(x):
    return (x + 15) & ~15


def restated(n_nodes, depth, n, f16, global_nodes, lds_geom, fmt, geom, tris, large1):
    """The shim's layout of a BVH launch as it stood in render_enqueue_impl, step by step: lay out for 256 threads, ask which build that is,
    and re-lay a large one.  geom: the request's build has the GEOM stage; large1: its NODES == 1 build is a 768-thread one.
    -> (nodes, format, block, stack_off, geom_off, tri_off, bytes)"""
    ldsn = f16 and not global_nodes
    levels = max(depth + 3, 4)
    off = align16(n_nodes * 32) if ldsn else 0
    stack_off, geom_off = off, 0
    off = align16(off + levels * BLOCK * (2 if ldsn else 4))
    if ldsn:
        in_lds = off + n * 16 <= CU_LDS // (1536 // BLOCK)
        if lds_geom >= 0:
            in_lds = lds_geom != 0 and n <= LDS_GEOM_MAX
        if fmt == 2:
            in_lds = False
        if in_lds and not geom:
            geom_off = off
            off += n * 16
    size = off
    nodes = (2 if geom_off else 1) if ldsn else 0
    block = BLOCK_LARGE if nodes == 1 and large1 else BLOCK
    node_format = 1 if ldsn else 0
    if block != BLOCK:
        stack = align16(levels * block * 2)
        bytes32 = n_nodes * 28 * 4
        one, two = f16 and bytes32 + stack <= CU_LDS, f16 and 2 * (bytes32 + stack) <= CU_LDS
        if one if fmt == 2 else (fmt == 0 and two):
            stack_off, size, node_format = bytes32, bytes32 + stack, 2
        else:
            geom_off, size, nodes, block = off, off + n * 16, 2, BLOCK
    tri_off = 0
    if tris:
        tri_off = align16(size)
        size = tri_off + 16
    return nodes, node_format, block, stack_off, geom_off, tri_off, size


def got(c):
    nodes = int(c["build"].split("<")[1].split(",")[1]) if c["build"].startswith("render_bvh") else None
    return nodes, c["node_format"], c["block"], c["lds_stack_off"], c["lds_geom_off"], c["lds_tri_off"], c["lds_bytes"]


@pytest.mark.parametrize("n_leaves", [2, 3, 6, 100, 481, 500, 512, 513])
def test_layout_is_the_restated_rule(n_leaves):
    """Trees with f16 nodes at every depth from balanced to the builder's cap, trees without at RTW_BVH_STACK; scenes of the tree's
    spheres alone, with one big sphere, and at and just past RTW_LDS_GEOM_MAX; every value of the two options; a request with and
    without triangles, quads, a moving sphere and RTW_FLAG_GLOBAL_NODES, in the common configuration (whose static NODES == 1 build is a
    768-thread one) and presentation_image's (256 threads)."""
    balanced = math.ceil(math.log2(n_leaves))
    n_nodes = n_leaves - 1
    for n in sorted({n_leaves, n_leaves + 1, LDS_GEOM_MAX, LDS_GEOM_MAX + 1}):
        if n < n_leaves:
            continue
        depths = {True: range(balanced, expected_cap(n_leaves, min(n, LDS_GEOM_MAX), 0.0) + 1), False: (STACK,)}
        for f16 in (True, False):
            for depth, lds_geom, fmt in itertools.product(depths[f16], (-1, 0, 1), (0, 1, 2)):
                t = tree(n_nodes, depth, n, f16)
                for config, tris, quads, moving, glob in itertools.product((COMMON, DEMO), (0, 1), (0, 1), (False, True), (False, True)):
                    f = facts(flags=R.FLAG_GLOBAL_NODES if glob else 0, n_triangles=tris, n_quads=quads, **config)
                    c = R.render_choice(f, t, lds_geom=lds_geom, node_format=fmt, moving=moving)
                    geom = bool(tris or quads)
                    spec = 8 if tris else (2 if quads else 1) if config is COMMON else 4
                    what = (n_leaves, n, f16, depth, lds_geom, fmt, config is COMMON, tris, quads, moving, glob)
                    nodes = got(c)[0]
                    assert c["build"] == B.bvh(moving, nodes, spec, geom), what
                    assert got(c) == restated(n_nodes, depth, n, f16, glob, lds_geom, fmt, geom, tris, B.bvh(moving, 1, spec, geom) in LARGE_BUILDS), what
                    assert all(c[k] % 16 == 0 for k in ("lds_stack_off", "lds_geom_off", "lds_tri_off", "lds_bytes")) and c["lds_bytes"] <= CU_LDS, what
                    assert (c["block"] == BLOCK_LARGE) == (c["node_format"] == 2) == (c["build"] in LARGE_BUILDS), what
                    if c["node_format"] == 2 and fmt == 0:
                        assert 2 * c["lds_bytes"] <= CU_LDS, what                  # two workgroups fit a CU
                    if nodes == 2:
                        assert not geom and c["lds_geom_off"] > c["lds_stack_off"], what
                    else:
                        assert c["lds_geom_off"] == 0, what
                    assert (c["lds_tri_off"] != 0) == bool(tris), what


def test_the_list_walk_has_no_lds_but_the_triangle_counter():
    for tris, moving, glob in itertools.product((0, 7), (False, True), (False, True)):
        c = R.render_choice(facts(flags=R.FLAG_GLOBAL_NODES if glob else 0, n_triangles=tris, **COMMON), tree(480, 14, 485), lds_geom=1,
                            moving=moving, accel=R.ACCEL_BRUTE)
        assert got(c) == (None, 0, BLOCK, 0, 0, 0, 16 if tris else 0) and c["build"] == B.brute(moving, 8 if tris else 1, bool(tris))
