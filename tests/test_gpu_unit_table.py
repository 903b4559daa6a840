"""The unit table of the 768-thread render builds (csrc/rtw_kernels.hip fetch_pixel<true>): at every block decode lane l of the wave
computes {column | row << 16, hash of (seed, pixel)} of pixel l of the block's tile, and a lane that takes unit p pulls entry p from
lane p instead of computing it.

Every case renders the suite's small view of Book-1's final scene (gamma 1, depth 6) right after a poison render in the same context and
is the CPU oracle's frame bit for bit, with camera_rays == width x height x samples and the oracle's segments.  No tolerances.  The
shapes are the smallest at which the table can go wrong: padding entries, pulls from lanes that do not ask under every refill pattern
(units of one sample, so a two- or five-block grab straddles tiles and the table is rebuilt while lanes still trace the previous tile's
units), the row map of a partition inside the table, rows above 2^12 in `row << 16`, and the end of the queue.

Two mutations of the kernel, each built once and run against this file, not kept (DESIGN.md 4.0 names the cases that catch each): the
pulls moved inside the lane region of the asking lanes, and the table rebuilt only at a grab instead of at every block."""
import functools

import numpy as np
import pytest

import rtw_amd as R
from tests import builds_common as B
from tests import oracle_binding as O
from tests import queue_common as Q
from tests.test_oracle_golden import small_view

pytestmark = pytest.mark.gpu
LARGE = {B.bvh(0, 1, 1, 0), B.bvh(0, 1, 2, 0), B.bvh(0, 1, 3, 0)}       # the builds whose workgroup is 768 threads
C, G, S, P = R.OPT_CHUNK_LEN, R.OPT_GRAB_BLOCKS, R.OPT_SUB_QUEUES, R.OPT_BLOCKS_PER_CU


def view(w, h, spp):
    """Q.view for a frame of any size: small_view accepts every size from one pixel up, so the frames below one tile are used as named."""
    scene, cam, p = small_view(R.SCENE_C2, w, h, spp)
    p.gamma, p.depth, p.flags = 1.0, Q.DEPTH, 0
    return scene, cam, p


@functools.lru_cache(maxsize=None)
def oracle(w, h, spp):
    """(frame, RtwStats) of the CPU oracle, once per process, read-only."""
    scene, cam, p = view(w, h, spp)
    img, st = O.render(cam, scene, p, Q.THREADS)
    img.setflags(write=False)
    return img, st


@pytest.fixture(scope="module")
def ctx(rtw):
    assert rtw.device_count() > 0, "no HIP device visible: -m gpu tests need the MI355X"
    with rtw.Renderer(0) as r:
        r.set_scene(R.Scene.generate(R.SCENE_C2))
        yield r


def run(r, w, h, spp, kind="bvh768", opts=(), partition=None):
    """Render the frame part by part, each right after a poison render; build, counters and bits.  Returns the plans of the last part."""
    ref, st_ref = oracle(w, h, spp)
    frame = np.full((h, w, 3), np.nan, np.float32)
    rays = segments = 0
    try:
        for k, v in dict(opts).items():
            r.set_option(k, v)
        for i in range(partition[1] if partition else 1):
            _, cam, p = view(w, h, spp)
            p.flags = Q.BUILD_KINDS[kind][1]
            p.accel = Q.BUILD_KINDS[kind][0]
            p.row_block, p.part_index, p.part_count = (partition[0], i, partition[1]) if partition else (8, 0, 1)
            rows = Q.part_rows(h, p.row_block, i, p.part_count)
            bad = Q.poison(r, cam, p)
            img, st = r.render(cam, p)
            build = r.last_render_build()
            assert build == Q.build_choice(kind)["build"], (kind, build)
            assert (build in LARGE) == (kind == "bvh768"), (kind, build)
            assert img.shape == bad.shape == (len(rows), w, 3)
            frame[rows] = img
            rays += st.camera_rays
            segments += st.segments
        plans = [r.last_queue_plan(b) for b in range(r.last_queue_bands())]
    finally:
        for k, v in Q.DEFAULTS.items():
            r.set_option(k, v)
    assert rays == w * h * spp and segments == st_ref.segments, (rays, segments, st_ref.segments)
    wrong = (frame.view(np.uint32) != ref.view(np.uint32)).any(axis=2)
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:4].tolist())
    return plans


@pytest.mark.parametrize("w,h", [(5, 3), (9, 9), (70, 67)])
def test_padding_entries(ctx, w, h):
    """One tile with 15 valid of 64 entries, four tiles of which three are ragged, 81 tiles with a ragged last column and row: 3 spp."""
    (q,) = run(ctx, w, h, 3)
    assert q["n_tiles"] == Q.cdiv(w, 8) * Q.cdiv(h, 8) and q["block"] == 768, q


@pytest.mark.parametrize("grab", [1, 2, 5])
@pytest.mark.parametrize("w,h", [(24, 16), (72, 56)])
def test_pulls_under_every_refill_pattern(ctx, w, h, grab):
    """Units of one sample at 3 spp, three blocks per tile, under RTW_OPT_GRAB_BLOCKS 1, 2 and 5.  6 and 63 tiles: single queues.  (At this
    size every grab is one block whatever the option allows -- see MANY below for the frames on which grabs straddle tiles.)"""
    (q,) = run(ctx, w, h, 3, opts={C: 1, G: grab})
    assert q["n_chunks"] == 3 and q["grab_max"] == 64 * min(grab, 3) and q["sub_shift"] == 0, q


@pytest.mark.parametrize("sub_queues", [0, 1])
@pytest.mark.parametrize("grab", [1, 2, 5])
def test_pulls_with_one_and_eight_sub_queues(ctx, grab, sub_queues):
    """The same on a frame that has 64 tiles and 64 workgroups of 768 threads: 104 x 40 (65 tiles) at 12 spp in units of one sample, 780
    blocks.  RTW_OPT_SUB_QUEUES 0 gives eight sub-queues there, 1 a single one."""
    (q,) = run(ctx, 104, 40, 12, opts={C: 1, G: grab, S: sub_queues})
    assert q["n_tiles"] == 65 and q["n_chunks"] == 12 and q["grab_max"] == 64 * grab and q["grid"] >= 64, q
    assert q["sub_shift"] == (3 if sub_queues == 0 else 0), q


# The frames above are sized by the work: the grid is capped at one workgroup per 768 items, so every wave takes one block, with all of its
# lanes asking at once, and a grab -- what is left >> grab_shift, in whole blocks -- never reaches two blocks.  A wave holds several blocks
# one after the other, with its lanes drifted apart, and a grab spans two or three blocks, only when total_work >> grab_shift >= 128:
# with 256 workgroups of twelve waves (RTW_OPT_BLOCKS_PER_CU 1 on an MI355X) grab_shift is 14, or 11 with eight sub-queues, and that is
# 2.1 M units of one sample.  These are the smallest such frames: an odd number of blocks per tile, so grabs of two straddle tiles.
MANY = {"single63": (72, 56, 523), "t65": (104, 40, 803)}      # 63 tiles: a single queue whatever the option; 65 tiles: eight sub-queues


def run_many(ctx, name, grab, sub_queues):
    w, h, spp = MANY[name]
    (q,) = run(ctx, w, h, spp, opts={C: 1, G: grab, S: sub_queues, P: 1})
    assert q["n_chunks"] == spp and q["grab_max"] == 64 * grab and q["block"] == 768 and q["grid"] * 768 * 8 < q["total_work"], q
    per_queue = q["total_work"] >> q["sub_shift"]                 # (about: the sub-queues differ by a tile)
    assert ((per_queue >> q["grab_shift"]) >= 128) and spp % 2 == 1, q      # the first grabs are of two blocks or more unless the option says one
    return q


@pytest.mark.parametrize("grab", [1, 2])
def test_drifted_lanes_and_straddling_grabs_single_queue(ctx, grab):
    """72 x 56 at 523 spp in units of one sample on one workgroup per CU: every wave works through ~11 blocks, in grabs of one or two."""
    q = run_many(ctx, "single63", grab, 0)
    assert q["sub_shift"] == 0, q


@pytest.mark.parametrize("sub_queues", [0, 1])
@pytest.mark.parametrize("grab", [1, 2, 5])
def test_drifted_lanes_and_straddling_grabs(ctx, grab, sub_queues):
    """104 x 40 at 803 spp likewise, ~17 blocks per wave, with eight sub-queues and with one; RTW_OPT_GRAB_BLOCKS 5 gives grabs of three
    blocks here (what is left >> grab_shift is 192 .. 203 at the start), and 803 is a multiple of neither two nor three."""
    q = run_many(ctx, "t65", grab, sub_queues)
    assert q["sub_shift"] == (3 if sub_queues == 0 else 0), q


@pytest.mark.parametrize("part_count", [2, 3])
@pytest.mark.parametrize("row_block", [1, 3, 8, 16])
def test_row_map_inside_the_table(ctx, row_block, part_count):
    """Row blocks of 1, 3, 8 and 16 rows dealt to two and three parts of 40 x 48 at 2 spp, every part: the parts put together are the frame."""
    run(ctx, 40, 48, 2, partition=(row_block, part_count))


@pytest.mark.parametrize("partition", [None, (8, 3)], ids=["whole", "3 parts"])
def test_rows_above_4096(ctx, partition):
    """8 x 4099 at 1 spp, 513 tiles: `row << 16` with rows up to 4098, whole and as three parts in blocks of 8 rows."""
    plans = run(ctx, 8, 4099, 1, partition=partition)
    if partition is None:
        assert sum(q["n_tiles"] for q in plans) == 513, plans


def test_queue_end_most_waves_find_nothing(ctx):
    """8 x 8 at 1 spp under RTW_OPT_BLOCKS_PER_CU 0: one block of work for a workgroup of twelve waves."""
    (q,) = run(ctx, 8, 8, 1, opts={P: 0})
    assert q["total_work"] == 64 and q["grid"] == 1 and q["block"] == 768, q


def test_queue_end_two_block_grab(ctx):
    """16 x 8 at 1 spp with RTW_OPT_GRAB_BLOCKS 2: two blocks in the whole queue."""
    (q,) = run(ctx, 16, 8, 1, opts={G: 2})
    assert q["total_work"] == 128, q


@pytest.mark.parametrize("kind", ["bvh256", "brute"])
def test_other_builds_are_what_they_were(ctx, kind):
    """A 256-thread tree build and the list walk on 70 x 67 at 3 spp: they keep the per-lane tail."""
    (q,) = run(ctx, 70, 67, 3, kind=kind)
    assert q["block"] == 256, q
