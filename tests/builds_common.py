"""The compiled builds of the render kernels by name: render_brute<MOVING, SPEC, GEOM> and render_bvh<MOVING, NODES, SPEC, GEOM>
(csrc/rtw_kernels.hip), written as Renderer.last_render_build() writes them -- "render_brute<0,4,1>", "render_bvh<1,2,5,0>".

A test module that enumerates builds exports a module-level table BUILDS of the tags its cases declare, and every case asserts that the
render it made ran the tag it declared.  tests/test_render_builds_cpu.py reads the list of compiled builds from librtw_hip.so and holds
the union of the tables (CLAIMING) against it: a build nobody claims, or a claim for a build that is not compiled, fails there, on the
CPU."""
import re

import rtw_amd as R

# the test modules whose BUILDS tables together must be the library's list
CLAIMING = ("tests.test_gpu_round2", "tests.test_gpu_render_builds", "tests.test_gpu_oracle_tri_noise", "tests.test_gpu_lights")

# the host side registers each kernel under its Itanium-mangled name, a plain string in the library file:
# _ZN3rtw10render_bvhILb1ELi2ELi5ELb0EEEvNS_5KArgsE = void rtw::render_bvh<true, 2, 5, false>(rtw::KArgs)
MANGLED = re.compile(rb"_ZN3rtw(?:10render_bvhILb([01])ELi(\d+)ELi(\d+)ELb([01])E|12render_bruteILb([01])ELi(\d+)ELb([01])E)EEvNS_5KArgsE")


def brute(moving, spec, geom):
    return f"render_brute<{int(moving)},{int(spec)},{int(geom)}>"


def bvh(moving, nodes, spec, geom):
    return f"render_bvh<{int(moving)},{int(nodes)},{int(spec)},{int(geom)}>"


def tag(moving, nodes, spec, geom):
    """nodes None: the list walk; 0 / 1 / 2: the tree with f32 nodes in global memory / f16 nodes in LDS / LDS nodes and LDS spheres."""
    return brute(moving, spec, geom) if nodes is None else bvh(moving, nodes, spec, geom)


def family(spec, geom, moving=(False, True), nodes=None):
    """The tags of one SPEC: the list walk and the tree at each of `nodes` (default: 0, 1 with GEOM, 0, 1, 2 without), for each `moving`."""
    if nodes is None:
        nodes = (None, 0, 1) if geom else (None, 0, 1, 2)
    return frozenset(tag(m, n, spec, geom) for m in moving for n in nodes)


def library_builds(path=None):
    """Every render_brute / render_bvh instantiation named in the library file, as tags."""
    data = open(path or R.LIB_PATH, "rb").read()
    out = set()
    for m in MANGLED.finditer(data):
        if m.group(1) is not None:
            out.add(bvh(m.group(1) == b"1", int(m.group(2)), int(m.group(3)), m.group(4) == b"1"))
        else:
            out.add(brute(m.group(5) == b"1", int(m.group(6)), m.group(7) == b"1"))
    return out


def ran(renderer, want, what=""):
    """The one assertion every enumerating case makes after a render: it ran the build it declared."""
    got = renderer.last_render_build()
    assert got == want, (what, got, want)
