"""The render work queue on the host alone (tests/queue_common.py): the restated plan and decode hand out every (tile, sample) and every
bank slot exactly once over a sweep of plans that visits every threshold of the arithmetic; every case of the GPU table (test_gpu_queue.py)
engages the path it is named for on an MI355X, with the workgroup sizes the library compiles today; the statuses of
rtw_ctx_last_queue_plan that need no device."""
import ctypes as C
import itertools

import numpy as np
import pytest

import rtw_amd as R
from tests import builds_common as B
from tests import queue_common as Q

# tile counts: the small ones, around the sub-queue threshold (63 / 64 / 65), around 128; none but 8, 16, 64, 72, 128 a multiple of 8
TILES = tuple(range(1, 20)) + tuple(range(62, 74)) + (127, 128, 129)
SAMPLES = (1, 2, 3, 4, 5, 7, 8, 12, 13, 16, 25, 64)
LENGTHS = (1, 2, 3, 4, 5, 6, 7, 11, 12, 13)                  # the thresholds 5 / 6 and 11 / 12 of L2; 0 (auto) is a choice among these
TAILS = (0.0, 0.5, 1.0, 2.0, 64.0)
# (workgroups the device offers, threads per workgroup): one and several per CU of an MI355X, and offers of 63 / 64 so that the sub-queue
# rule's grid threshold is met from both sides by the offer as well as by the cap
GRIDS = ((256, 256), (256, 768), (512, 256), (2048, 256), (63, 256), (64, 256), (64, 768))


def test_the_sweep_visits_every_threshold():
    """What the partition test below relies on: the swept plans include each edge by name."""
    seen = set()
    for n_tiles, n, L, k, (g, blk), sq in itertools.product((63, 64, 65, 81), SAMPLES, LENGTHS, TAILS, GRIDS, (0, 1)):
        q = Q.expected_plan(n_tiles, n, L, k, g, blk, sq, 2, False)
        seen.add(("sub", n_tiles, min(q["grid"], 65) if q["grid"] in (63, 64, 65) else 0, q["sub_shift"]))
        if q["reg_q2"] < n_tiles:
            seen.add(("L2", L, q["reg_len"][1]))
            seen.add(("ragged", 0, n % q["reg_len"][0] != 0))
            if q["reg_q1"] < q["reg_q2"]:
                seen.add(("ragged", 1, n % q["reg_len"][1] != 0))
                if q["sub_shift"] and q["reg_q1"] % 8 and q["reg_q2"] % 8:
                    seen.add("bounds%8")
    for n_tiles in (63, 64, 65):
        assert ("sub", n_tiles, 64, 3 if n_tiles >= 64 else 0) in seen and ("sub", n_tiles, 63, 0) in seen, n_tiles      # 63 / 64 workgroups x 63 / 64 / 65 tiles
    assert {("L2", 5, 1), ("L2", 6, 2), ("L2", 11, 2), ("L2", 12, 4)} <= seen
    assert {("ragged", 0, True), ("ragged", 0, False), ("ragged", 1, True), ("ragged", 1, False), "bounds%8"} <= seen


def test_every_plan_of_the_sweep_is_a_partition():
    """285 600 plans (and the chunk-sum layout of each tile count and sample count): every (queue position, sample) exactly once, every
    bank slot exactly once, no empty unit, the sub-queues' items add up to total_work.  Plans that are the same partition -- equal in what
    the decode reads -- are checked once."""
    done, n_plans = set(), 0
    for n_tiles, n, L, k, (g, blk), sq in itertools.product(TILES, SAMPLES, LENGTHS, TAILS, GRIDS, (0, 1)):
        q = Q.expected_plan(n_tiles, n, L, k, g, blk, sq, 2, False)
        n_plans += 1
        key = Q.partition_key(q)
        if key not in done:
            done.add(key)
            Q.assert_partition(q)
    assert n_plans == 285600 and len(done) > 5000, (n_plans, len(done))
    for n_tiles, n, (g, blk), sq in itertools.product(TILES, SAMPLES, GRIDS, (0, 1)):
        q = Q.expected_plan(n_tiles, n, 7, 2.0, g, blk, sq, 2, True)
        assert q["bank_len"] == 1 and q["chunk_len"] == min(4, n) and q["reg_q1"] == q["reg_q2"] == n_tiles
        Q.assert_partition(q)


def test_assert_partition_sees_a_wrong_plan():
    """The checker itself: a plan whose regions or totals are off by one is refused."""
    good = Q.expected_plan(81, 25, 6, 2.0, 256, 256, 0, 2, False)
    Q.assert_partition(good)
    for field, delta in (("total_work", 64), ("n_tiles", 1), ("n_tiles", -1), ("n_samples", 1)):
        bad = dict(good, **{field: good[field] + delta})
        with pytest.raises(AssertionError):
            Q.assert_partition(bad)
    bad = dict(good, reg_nc=[good["reg_nc"][0], good["reg_nc"][1] - 1, good["reg_nc"][2]])
    with pytest.raises(AssertionError):
        Q.assert_partition(bad)


def test_the_block_sizes_are_read_not_assumed():
    """The three kinds of build the cases run, as rtw_render_choice describes them today: the names of builds_common and 256 / 256 / 768
    threads.  A change of bvh_block or of render_brute's launch bounds shows here, and every property below follows the new size."""
    blocks = {}
    for kind in Q.BUILD_KINDS:
        for flags in (0, R.FLAG_CHUNK_SUMS, R.FLAG_CHUNK_SUMS | Q.GENERIC):
            c = Q.build_choice(kind, flags)
            want = Q.build_tag(kind, flags)
            assert want is None or c["build"] == want, (kind, flags, c)
            assert c["build"] in B.library_builds(), c
            blocks[kind, flags] = c["block"]
    assert blocks["brute", 0] == 256 and blocks["bvh256", 0] == 256 and blocks["bvh768", 0] == 768, blocks
    assert blocks["bvh768", R.FLAG_CHUNK_SUMS] == 768 and blocks["bvh256", R.FLAG_CHUNK_SUMS | Q.GENERIC] == 256, blocks
    assert Q.build_choice("bvh256", R.FLAG_CHUNK_SUMS | Q.GENERIC)["build"] == B.bvh(0, 0, 0, 0)
    assert Q.build_choice("bvh256", R.FLAG_CHUNK_SUMS)["build"] == B.bvh(0, 0, 3, 0)


@pytest.mark.parametrize("case", Q.CASES, ids=lambda c: c.id)
def test_every_case_engages_its_path_on_an_mi355x(case):
    """expected_plan for the case on 256 CUs, with the workgroup size its build compiles to: the plan shows what the case is named for (a case
    that cannot engage its path fails here, not silently on the GPU), and is a partition."""
    parts = range(case.partition[1]) if case.partition else (0,)
    for i in parts:
        plans = Q.case_plans(case, part_index=i)
        assert plans, case.id
        Q.assert_shows(case, plans)
        for q in plans:
            Q.assert_partition(q)


def test_the_table_covers_what_it_is_there_for():
    """Both untested options are set by cases, every group is present, and the edges of the arithmetic each occur in some case's plan."""
    groups = {c.group for c in Q.CASES}
    assert groups == set("ABCDEGHI"), groups                       # (F, explicit grids, and J, the accessor's statuses, are tests of their own)
    assert any(c.opts.get(R.OPT_SUB_QUEUES) == 1 for c in Q.CASES)
    shown = set()
    for c in Q.CASES:
        for s in c.shows:
            shown.update(s)
    assert {"subq8", "single", "tiles%8", "region2 empty", "both capped", "bounds%8", "ragged r1", "ragged r2", "L2=1", "L2=2", "L2=4",
            "grab tile", "grab 5", "tile order", "sums", "block 768", "grid<64"} <= shown
    # bands of one render with sub-queues and without
    assert any(len(c.shows) == 3 and "subq8" in c.shows[0] and "single" in c.shows[2] for c in Q.CASES)
    # a partition in blocks other than 8 rows with eight sub-queues
    assert any(c.partition and c.partition[0] != 8 and "subq8" in c.shows[0] for c in Q.CASES)


def test_explicit_grids_on_an_mi355x():
    """Case F's arithmetic: RTW_OPT_BLOCKS_PER_CU = v gives v x 256 workgroups up to the cap, at least three different grids for either
    size of workgroup."""
    for block in (256, 768):
        grids = []
        for v in Q.GRID_VALUES:
            q = Q.expected_plan(128, Q.GRID_SPP, 1, 0.0, Q.device_grid(Q.MI355X_CUS, block, 128, Q.GRID_SPP, v), block, 0, 2, False)
            assert q["grid"] == min((v or 1) * 256, Q.cdiv(128 * 64 * 64, block)) and q["sub_shift"] == 3
            grids.append(q["grid"])
        assert len(set(grids)) >= 3 and grids[0] == grids[-1] == 256, grids


@pytest.mark.parametrize("frame,spp", [("t63", 25), ("t64", 12), ("t65", 13), ("ragged81", 13), ("wide", 64), ("banded", 8)])
def test_the_poison_frame_is_wrong_almost_everywhere(frame, spp):
    """What a poison render leaves in the bank and the output buffer: the oracle's frame of the other seed differs from the expected one
    in at least 99 % of the pixels that are not pure background (at the fewest samples the frame is used with: more samples differ more)."""
    assert Q.poison_differs(frame, spp) >= 0.99
    assert Q.poison_differs(frame, spp, R.FLAG_CHUNK_SUMS) >= 0.99


def test_accessor_statuses_without_a_device():
    L = R.lib()
    q = R.RtwQueuePlan()
    assert C.sizeof(R.RtwQueuePlan) == 27 * 4
    assert L.rtw_ctx_last_queue_plan(None, 0, C.byref(q)) == -1          # RTW_E_INVALID: no context
    assert L.rtw_ctx_last_queue_plan(None, 0, None) == -1                # ... and nowhere to write
    assert all(v == 0 or v == [0, 0, 0] for v in q.as_dict().values())   # nothing was written
