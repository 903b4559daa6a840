"""The work queue of the persistent render kernels on the device: every case of tests/queue_common.py renders the CPU oracle's frame bit
for bit, right after a poison render in the same context, with the plan the library reports equal to the restated one, a partition, and
showing the path the case is named for.  No tolerances: `camera_rays`, `segments` and every bit of the frame.

The reference everywhere is the oracle's frame of the suite's small view of Book-1's final scene (gamma 1, depth 6), computed once per
(frame, samples, image-defining flags) and handed out read-only."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests import builds_common as B
from tests import queue_common as Q
from tests.render_limits_common import bank_gb_for_band

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(rtw):
    assert rtw.device_count() > 0, "no HIP device visible: -m gpu tests need the MI355X"
    with rtw.Renderer(0) as r:
        r.set_scene(R.Scene.generate(R.SCENE_C2))
        yield r


def set_options(r, opts):
    for k, v in opts.items():
        r.set_option(k, v)


def reset_options(r):
    set_options(r, Q.DEFAULTS)


def params_of(frame, spp, kind, flags, partition=None, part_index=0):
    _, cam, p = Q.view(frame, spp, flags | Q.BUILD_KINDS[kind][1])
    p.accel = Q.BUILD_KINDS[kind][0]
    p.row_block, p.part_index, p.part_count = (partition[0], part_index, partition[1]) if partition else (8, 0, 1)
    return cam, p


def plans_of(r):
    return [r.last_queue_plan(b) for b in range(r.last_queue_bands())]


@pytest.fixture(scope="module")
def device_cus(ctx):
    """The CUs of this device, read from a reported grid: RTW_OPT_BLOCKS_PER_CU = 1 is one workgroup per CU, and on `wide` at 64 spp in
    units of one sample the cap (2048 workgroups of 256 threads) does not bind -- asserted, so that the figure is the device's."""
    cam, p = params_of(Q.GRID_FRAME, Q.GRID_SPP, "bvh256", 0)
    try:
        set_options(ctx, {R.OPT_CHUNK_LEN: 1, R.OPT_BLOCKS_PER_CU: 1})
        ctx.render(cam, p)
        q = ctx.last_queue_plan(0)
    finally:
        reset_options(ctx)
    assert q["block"] == 256 and q["total_work"] == 128 * 64 * 64 and q["grid"] < q["total_work"] // q["block"], q
    return q["grid"]


def run_case(r, c, n_cu):
    """Render a case part by part, each right after a poison render; plans, counters and bits against the model and the oracle."""
    w, h = Q.FRAMES[c.frame]
    ref, st_ref = Q.oracle(c.frame, c.spp, c.flags)
    opts = dict(c.opts)
    if c.band_rows:
        sums = bool(c.flags & R.FLAG_CHUNK_SUMS)
        slots = Q.cdiv(c.spp, Q.SUM_CHUNK) if sums else c.spp
        opts[R.OPT_SAMPLE_BANK_GB] = bank_gb_for_band(Q.cdiv(w, 8), slots, c.band_rows)
    frame = np.full((h, w, 3), np.nan, np.float32)
    rays = segments = 0
    try:
        set_options(r, opts)
        for i in range(c.partition[1] if c.partition else 1):
            cam, p = params_of(c.frame, c.spp, c.kind, c.flags, c.partition, i)
            bad = Q.poison(r, cam, p)
            img, st = r.render(cam, p)
            got = plans_of(r)
            assert r.last_render_build() == Q.build_choice(c.kind, c.flags)["build"], (c.id, r.last_render_build())
            want = Q.case_plans(c, n_cu, part_index=i)
            assert got == want, (c.id, i, got, want)
            for q in got:
                Q.assert_partition(q)
            Q.assert_shows(c, got)
            rows = Q.part_rows(h, p.row_block, i, p.part_count)
            assert img.shape == bad.shape == (len(rows), w, 3)
            frame[rows] = img
            rays += st.camera_rays
            segments += st.segments
    finally:
        reset_options(r)
    assert rays == w * h * c.spp and segments == st_ref.segments, (c.id, rays, segments, st_ref.segments)
    wrong = (frame.view(np.uint32) != ref.view(np.uint32)).any(axis=2)
    assert not wrong.any(), (c.id, int(wrong.sum()), np.argwhere(wrong)[:4].tolist())


@pytest.mark.parametrize("case", Q.by_group("A"), ids=lambda c: c.id)
def test_sub_queue_threshold(ctx, device_cus, case):
    """63 / 64 / 65 / 81 tiles and 48 / 64 workgroups under RTW_OPT_SUB_QUEUES 0 and 1: eight sub-queues exactly from 64 tiles and 64
    workgroups under option 0."""
    run_case(ctx, case, device_cus)


@pytest.mark.parametrize("case", Q.by_group("B"), ids=lambda c: c.id)
def test_regions_and_sub_queues(ctx, device_cus, case):
    """RTW_OPT_TAIL_UNITS 0.5 / 2 / 64 x unit lengths 5, 6, 11, 12, 13 x 13 and 25 spp x both sub-queue settings on 81 tiles: region 2 empty
    at length 5, both regions capped at a quarter of the tiles at k = 64, boundaries that are no multiple of 8, ragged last chunks."""
    run_case(ctx, case, device_cus)


@pytest.mark.parametrize("case", Q.by_group("C"), ids=lambda c: c.id)
def test_grabs(ctx, device_cus, case):
    """RTW_OPT_GRAB_BLOCKS 0 / 1 / 2 / 5 with 13 blocks per tile: grabs cross tile and region boundaries."""
    run_case(ctx, case, device_cus)


@pytest.mark.parametrize("case", Q.by_group("D"), ids=lambda c: c.id)
def test_tile_orders(ctx, device_cus, case):
    """RTW_OPT_TILE_ORDER 1 .. 5 with eight sub-queues and three regions: the order is handed over and only renames the tiles."""
    run_case(ctx, case, device_cus)


@pytest.mark.parametrize("case", Q.by_group("E"), ids=lambda c: c.id)
def test_build_sizes(ctx, device_cus, case):
    """The list walk, a 256-thread and the 768-thread tree build, by the names of builds_common: the 768-thread one reaches 64 workgroups
    three times later, so its cases are larger -- and one stays a single queue."""
    run_case(ctx, case, device_cus)
    want = Q.build_tag(case.kind, case.flags)
    assert want in (B.brute(0, 1, 0), B.bvh(0, 0, 1, 0), B.bvh(0, 1, 1, 0))
    assert Q.build_choice(case.kind, case.flags)["build"] == want          # (run_case held the render to the choice)


def test_explicit_grid(ctx, device_cus):
    """RTW_OPT_BLOCKS_PER_CU 1, 2, 3, 6, 8, then 0 again, on 128 tiles x 64 units of one sample, with both sizes of workgroup: the grid is v
    x the CUs up to the cap, at least three grids occur, the frame is the oracle's every time.

    A grid above what is resident is only a longer launch: no workgroup of render_brute or render_bvh waits for another one.  Read in
    csrc/rtw_kernels.hip: the only traffic between workgroups is atomicAdd -- on the sub-queue counters in fetch_pixel, whose return value
    a wave uses at once and never polls, and on the statistics when a wave leaves --; there is no flag, fence or counter that a loop
    reads again, and both persistent loops end on the wave's own state (every lane found all sub-queues empty, or the trip valve).  The
    one barrier is the __syncthreads after a workgroup copies its tree into LDS, before its loop, inside the workgroup."""
    n_cu = device_cus
    ref, st_ref = Q.oracle(Q.GRID_FRAME, Q.GRID_SPP)
    for kind in ("bvh256", "bvh768"):
        block = Q.build_choice(kind)["block"]
        cam, p = params_of(Q.GRID_FRAME, Q.GRID_SPP, kind, 0)
        grids = []
        try:
            ctx.set_option(R.OPT_CHUNK_LEN, 1)
            for v in Q.GRID_VALUES:
                ctx.set_option(R.OPT_BLOCKS_PER_CU, v)
                Q.poison(ctx, cam, p)
                img, st = ctx.render(cam, p)
                (q,) = plans_of(ctx)
                want = Q.expected_plan(128, Q.GRID_SPP, 1, 0.0, Q.device_grid(n_cu, block, 128, Q.GRID_SPP, v), block, 0, 2, False)
                assert {k: q[k] for k in want} == want, (kind, v, q, want)
                assert q["grid"] == min((v or 1) * n_cu, Q.cdiv(q["total_work"], block)) and q["sub_shift"] == 3, (kind, v, q)
                Q.assert_partition(q)
                assert st.camera_rays == 128 * 64 * Q.GRID_SPP and st.segments == st_ref.segments, (kind, v)
                assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (kind, v)
                grids.append(q["grid"])
        finally:
            reset_options(ctx)
        assert len(set(grids)) >= 3 and grids[0] == grids[-1] == n_cu, (kind, grids)


@pytest.mark.parametrize("case", Q.by_group("G"), ids=lambda c: c.id)
def test_bands(ctx, device_cus, case):
    """Three bands of one render -- 64, 64 and 8 tiles --: the first two run eight sub-queues, the last a single one.  8 spp as planned: the
    256-thread tree build reaches 64 workgroups per band there (units of 2), so the sample count need not be raised."""
    run_case(ctx, case, device_cus)
    assert len(case.shows) == 3


@pytest.mark.parametrize("case", Q.by_group("H"), ids=lambda c: c.id)
def test_row_partitions(ctx, device_cus, case):
    """Row blocks of 1, 3, 8 and 16 rows dealt to three parts: the compact outputs put together are the oracle's whole frame.  Three
    parts of 81 tiles are below 64 tiles each -- single queues, still right --; two parts of the tall frame in blocks of 3 rows keep eight."""
    run_case(ctx, case, device_cus)


@pytest.mark.parametrize("case", Q.by_group("I"), ids=lambda c: c.id)
def test_chunk_sums(ctx, device_cus, case):
    """RTW_FLAG_CHUNK_SUMS against the oracle under the same flag: one bank slot per unit, the regions off whatever RTW_OPT_TAIL_UNITS
    says, RTW_OPT_CHUNK_LEN ignored; the build that folds the flag in and the generic one; banded and partitioned."""
    run_case(ctx, case, device_cus)


def test_accessor_statuses(rtw):
    """RTW_E_INVALID before the first render, for band == bands and for a NULL out; a refused render leaves the last record."""
    L = rtw.lib()
    with rtw.Renderer(0) as r:
        r.set_scene(R.Scene.generate(R.SCENE_C2))
        q = R.RtwQueuePlan()
        assert L.rtw_ctx_last_queue_plan(r._h, 0, C.byref(q)) == -1
        with pytest.raises(R.RtwError):
            r.last_queue_bands()
        cam, p = params_of("t65", 13, "bvh256", 0)
        r.render(cam, p)
        assert r.last_queue_bands() == 1
        first = r.last_queue_plan(0)
        assert first["n_tiles"] == 65 and first["n_samples"] == 13 and first["bands"] == 1
        assert L.rtw_ctx_last_queue_plan(r._h, 1, C.byref(q)) == -1           # band == bands
        assert L.rtw_ctx_last_queue_plan(r._h, 0, None) == -1
        bad = R.RtwParams.from_buffer_copy(p)
        bad.samples = 1 << 24                                                  # one more than a sampler may trace: refused
        with pytest.raises(R.RtwError):
            r.render(cam, bad)
        try:
            r.set_option(R.OPT_SAMPLE_BANK_GB, 1e-9)                           # less than one row of tiles: RTW_E_NOMEM
            with pytest.raises(R.RtwError):
                r.render(cam, p)
        finally:
            r.set_option(R.OPT_SAMPLE_BANK_GB, 48)
        assert r.last_queue_bands() == 1 and r.last_queue_plan(0) == first
