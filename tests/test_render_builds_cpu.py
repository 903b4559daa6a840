"""Which render kernels are compiled, read from librtw_hip.so itself, against which builds the suite's enumerations claim
(tests/builds_common.py) -- and the conditions on the inputs of tests/test_gpu_render_builds.py, checked with the oracle alone.  No GPU."""
import importlib

import numpy as np

import rtw_amd as R
from tests import builds_common as B
from tests import oracle_binding as O
from tests import render_builds_common as RB
from tests.test_gpu_scene_hits import oracle_hits


def tables():
    return {name: importlib.import_module(name).BUILDS for name in B.CLAIMING}


def test_tag_format_and_the_mangled_name_pattern():
    assert B.tag(True, 2, 5, False) == "render_bvh<1,2,5,0>" and B.tag(False, None, 4, True) == "render_brute<0,4,1>"
    blob = b"\0_ZN3rtw10render_bvhILb1ELi2ELi5ELb0EEEvNS_5KArgsE\0_ZN3rtw12render_bruteILb0ELi12ELb1EEEvNS_5KArgsE\0_ZN3rtw14resolve_kernelENS_5KArgsE\0"
    assert [m.group(0) for m in B.MANGLED.finditer(blob)] == [b"_ZN3rtw10render_bvhILb1ELi2ELi5ELb0EEEvNS_5KArgsE",
                                                              b"_ZN3rtw12render_bruteILb0ELi12ELb1EEEvNS_5KArgsE"]
    assert len(B.family(4, False)) == 8 and len(B.family(4, True)) == 6


def test_every_compiled_render_build_is_claimed_by_an_enumeration():
    """(a) every build the library holds is claimed by a table, (b) no table claims a build the library lacks, (c) no table is empty and
    the tables together claim each build at least once.  A pull request that adds or removes an instantiation fails here until a case of
    an enumerating test claims it (and asserts, on the GPU, that it ran it)."""
    compiled = B.library_builds()
    print(f"{len(compiled)} render kernels in {R.LIB_PATH}")
    assert len(compiled) >= 100 and B.brute(False, 0, False) in compiled and B.bvh(True, 2, 1, False) in compiled, sorted(compiled)[:8]
    claimed = tables()
    for name, t in claimed.items():
        assert len(t) > 0 and all(isinstance(x, str) for x in t), name
    union = set().union(*claimed.values())
    unclaimed = sorted(compiled - union)
    assert not unclaimed, f"compiled, but no enumeration runs them: {unclaimed}"
    phantom = {name: sorted(set(t) - compiled) for name, t in claimed.items() if set(t) - compiled}
    assert not phantom, f"claimed, but not in the library: {phantom}"
    counts = {b: sum(b in t for t in claimed.values()) for b in compiled}
    assert min(counts.values()) >= 1
    assert union == compiled


def test_the_new_enumeration_declares_one_case_per_tag_it_claims():
    mod = importlib.import_module("tests.test_gpu_render_builds")
    declared = [c[1] for c in RB.CASES]
    assert set(declared) == set(mod.BUILDS) and len(mod.BUILDS) == 54
    want = set()
    for spec in (4, 5, 6):
        want |= B.family(spec, False)
    for spec in (0, 2, 4, 5, 6):
        want |= B.family(spec, True)
    assert set(mod.BUILDS) == want


# ---- the inputs: conditions, not measurements ------------------------------------------------------------------------------------------
def test_inputs_scatter_and_motion_shows():
    """Every frame of a scattering integrator has more than 1.5 segments per camera ray (RTW_INTEGRATOR_NORMAL shades the first hit and
    cannot); the moving frame differs from the static one in at least 1 % of its pixels; every frame has all its pixels."""
    for geom in (False, True):
        for cfg in RB.CONFIGS[geom]:
            frames = {}
            for moving in (False, True):
                ref, st = RB.oracle_frame(geom, moving, cfg)
                n_samples = RB.SPP
                assert ref.shape == (RB.HEIGHT, RB.WIDTH, 3) and st.camera_rays == RB.WIDTH * RB.HEIGHT * n_samples, (geom, cfg[0], moving)
                if cfg[2] != R.INTEGRATOR_NORMAL:
                    assert st.segments > 1.5 * st.camera_rays, (geom, cfg[0], moving, st.segments, st.camera_rays)
                frames[moving] = ref
            differ = (~(frames[0].view(np.uint32) == frames[1].view(np.uint32)).all(axis=2)).mean()
            print(f"geom {geom} {cfg[0]}: {100 * differ:.1f} % of the pixels differ between the static and the moving frame")
            assert differ >= 0.01, (geom, cfg[0], differ)
            if cfg[3] == R.SAMPLER_ROW and not geom:
                # ... and not only because the two fields are laid out differently: under RTW_SAMPLER_ROW (the sampler that draws ray.time) the
                # moving field with its velocities taken away is another frame too
                scene, cam = RB.view(geom, True, cfg)
                still = R.Scene([scene._spheres[i] for i in range(scene.n_spheres)], textures=[scene._texels.reshape(4, 6, 3)], background=RB.BACKGROUND)
                for i in range(still.n_spheres):
                    still._spheres[i].velocity[1] = 0.0
                twin, _ = O.render(cam, still, RB.params(geom, True, cfg), threads=RB.THREADS, device_uv=True)
                moved = (~(twin.view(np.uint32) == frames[1].view(np.uint32)).all(axis=2)).mean()
                print(f"    {100 * moved:.1f} % of the pixels differ from the same field standing still")
                assert moved >= 0.01, (cfg[0], moved)


def test_geom_scene_shows_quads_box_and_spheres():
    """Quads, the box instance and the spheres are each the first hit of at least 2 % of the primary rays, static and moving; the wall
    quad has spheres in front of it (rays that would reach it end on a sphere first)."""
    for moving in (False, True):
        scene, cam = RB.view(True, moving, RB.SPHERE_CONFIGS[1])    # (depth_rays reads Rust2's camera; the Viewport's stands at the same place)
        rays = R.depth_rays(cam, RB.WIDTH, RB.HEIGHT)
        t, idx, _ = oracle_hits(O, scene, rays, cam.time0, 0.001, 1e30)
        ns, nq = scene.n_spheres, scene.n_quads
        share = {"spheres": np.mean((idx >= 1) & (idx < ns)), "quads": np.mean((idx >= ns) & (idx < ns + nq)), "box": np.mean(idx == ns + nq),
                 "medium": np.mean(idx == ns + nq + 1)}
        print(moving, {k: round(float(v), 4) for k, v in share.items()})
        for k in ("spheres", "quads", "box"):
            assert share[k] >= 0.02, (moving, k, share)
        assert share["medium"] > 0
        wall = R.Scene([], quads=[scene._quads[1]])
        tw, iw, _ = oracle_hits(O, wall, rays, cam.time0, 0.001, 1e30)
        hidden = (iw == 0) & (idx >= 1) & (idx < ns) & (t < tw)
        seen = idx == ns + 1
        assert hidden.sum() >= 20 and seen.sum() >= 20, (moving, int(hidden.sum()), int(seen.sum()))
