"""The work queue of the two persistent render kernels, restated in plain Python, and the cases that pin the compiled code to it
(test_queue_cpu.py, test_gpu_queue.py).

The queue decides which lane traces which (tile, chunk of samples, pixel) and into which bank slot the sample goes: the plan the shim
makes per band (csrc/rtw_shim.hip render_enqueue, from `a.k_base = tr0 * 8` to launch_render) and its decode in the kernels
(csrc/rtw_kernels.hip subq_layout, fetch_pixel).  Written from that code, in its order of steps, and independent of it at run time:

  expected_plan   the shim's rule for one band: unit length, grid cap, regions of unit length, sub-queues, guided grabs
  units_of        subq_layout and fetch_pixel's block decode: every 64-item block of every sub-queue -> (queue position, s0, s1, slot0)
  assert_partition  every (queue position, sample) once, every bank slot once

What a plan is compared with is what the library itself reports it launched (Renderer.last_queue_plan).  The one input the model cannot
know is how many workgroups the device offers; see device_grid.

The sample bank and the output buffer of a context are not cleared between renders, so a unit that is dropped, or a sample written to
another's slot, would leave the previous render's value where the resolve reads it: every GPU comparison is made right after a poison
render -- the same frame under the same options with another seed."""
import collections
import functools
import math

import numpy as np

import rtw_amd as R
from tests import builds_common as B
from tests import oracle_binding as O
from tests.test_oracle_golden import small_view

SUB_SHIFT = 3                       # RTW_SUB_SHIFT (csrc/rtw_kernels.h): eight sub-queues
SUM_CHUNK = 4                       # RTW_SUM_CHUNK (include/rtw.h)
MI355X_CUS = 256
THREADS = 16
DEPTH = 6
POISON_SEED = 0x9E3779B97F4A7C15    # xor-ed into the seed of a poison render
# the options a case may set, and what each goes back to (csrc/rtw_shim.hip struct rtw_ctx)
DEFAULTS = {R.OPT_CHUNK_LEN: 0, R.OPT_SAMPLE_BANK_GB: 48, R.OPT_BLOCKS_PER_CU: 0, R.OPT_TILE_ORDER: 0, R.OPT_GRAB_BLOCKS: 2, R.OPT_SUB_QUEUES: 0,
            R.OPT_TAIL_UNITS: 0.0}


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the shim's rule --------------------------------------------------------------------------------------------------------------------
def auto_chunk_len(frame_tiles, n_samples, n_cu):
    """RTW_OPT_CHUNK_LEN = 0: the unit length follows the size of the whole render (all bands)."""
    units4 = frame_tiles * cdiv(n_samples, 4) * 64
    lanes = n_cu * 1536
    if units4 >= 500 * lanes: return 12
    if units4 >= 200 * lanes: return 8
    if units4 >= 64 * lanes: return 6
    return 2 if units4 * 6 < 16 * lanes else 4


def unit_length(n_samples, chunk_len_option, sums, frame_tiles=None, n_cu=MI355X_CUS):
    """(chunk_len, n_chunks) of the queue's first region; RTW_FLAG_CHUNK_SUMS fixes the length, whatever the option says."""
    chunk_len = SUM_CHUNK if sums else chunk_len_option
    if chunk_len == 0:
        assert frame_tiles is not None, "RTW_OPT_CHUNK_LEN 0 needs the tiles of the whole render"
        chunk_len = auto_chunk_len(frame_tiles, n_samples, n_cu)
    chunk_len = min(chunk_len, n_samples)
    return chunk_len, cdiv(n_samples, chunk_len)


def device_grid(n_cu, block, n_tiles, n_chunks, blocks_per_cu_option=0, occupancy=None):
    """The persistent grid before the cap by the work: n_cu x workgroups per CU.  n_cu is a fact of the device: the GPU tests read it from
    the reported grid of a launch under RTW_OPT_BLOCKS_PER_CU = 1 that the cap does not bind (test_gpu_queue.py device_cus), the CPU tests
    use an MI355X's 256.  The workgroups per CU are the option, or min(occupancy, ceil(work / (16 items per lane of one workgroup per CU))):
    the occupancy the driver reports is needed only where that quotient exceeds 1 -- launches of more than n_cu x block x 16 items, none
    in these tests -- and must then be given."""
    if blocks_per_cu_option:
        return n_cu * blocks_per_cu_option
    total = n_tiles * n_chunks * 64
    want = max(cdiv(total, n_cu * block * 16), 1)
    if want == 1:
        return n_cu
    assert occupancy is not None, "a launch this large needs the kernel's occupancy"
    wg = min(occupancy, want)
    if wg > 6 and total < 40 * n_cu * 256 * wg:
        wg = 6
    return n_cu * wg


def expected_plan(n_tiles, n_samples, chunk_len_option, tail_units, grid_uncapped, block, sub_queues_option, grab_blocks_option, sums,
                  frame_tiles=None, n_cu=MI355X_CUS):
    """One band's plan as render_enqueue makes it: the fields of RtwQueuePlan that follow from these inputs."""
    chunk_len, n_chunks = unit_length(n_samples, chunk_len_option, sums, frame_tiles, n_cu)
    total = n_tiles * n_chunks * 64
    q1 = q2 = n_tiles
    reg_len, reg_nc = [chunk_len] * 3, [n_chunks] * 3
    grid = min(grid_uncapped, max(cdiv(total, block), 1))               # capped by the work of ONE unit length: the regions come after
    if not sums and tail_units > 0.0 and chunk_len > 1 and n_tiles > 1:
        waves = float(grid * (block // 64))
        L2 = 4 if chunk_len >= 12 else (2 if chunk_len >= 6 else 1)
        t3 = math.ceil(tail_units * waves * 1 / float(n_samples))
        t2 = math.ceil(tail_units * waves * L2 / float(n_samples)) if L2 > 1 else 0
        t3, t2 = min(t3, n_tiles // 4), min(t2, n_tiles // 4)
        q2 = n_tiles - t3
        q1 = q2 - t2
        reg_len[1], reg_len[2] = L2, 1
        reg_nc[1], reg_nc[2] = cdiv(n_samples, L2), n_samples
        total = (q1 * reg_nc[0] + (q2 - q1) * reg_nc[1] + (n_tiles - q2) * reg_nc[2]) * 64
    sub_shift = SUB_SHIFT if (sub_queues_option != 1 and n_tiles >= 64 and grid >= 64) else 0
    waves4 = (grid * (block // 64) * 4) >> sub_shift
    grab_shift = 0
    while grab_shift < 31 and (1 << grab_shift) < waves4:
        grab_shift += 1
    blocks = min(grab_blocks_option if grab_blocks_option else n_chunks, n_chunks)
    return dict(n_tiles=n_tiles, n_samples=n_samples, chunk_len=chunk_len, n_chunks=n_chunks, bank_len=1 if sums else 0, reg_q1=q1, reg_q2=q2,
                reg_len=reg_len, reg_nc=reg_nc, total_work=total, sub_shift=sub_shift, grab_shift=grab_shift, grab_max=max(blocks, 1) * 64,
                grid=grid, block=block)


# ---- the kernels' decode ----------------------------------------------------------------------------------------------------------------
def subq_layout(plan, sub):
    """SubQ of sub-queue `sub`: its tiles in region 1 / regions 1 + 2, the blocks before region 2 / 3, its items."""
    sh = plan["sub_shift"]
    up = (1 << sh) - 1 - sub
    t1, t2, t3 = (plan["reg_q1"] + up) >> sh, (plan["reg_q2"] + up) >> sh, (plan["n_tiles"] + up) >> sh
    b1 = t1 * plan["reg_nc"][0]
    b2 = b1 + (t2 - t1) * plan["reg_nc"][1]
    return dict(t1=t1, t2=t2, b1=b1, b2=b2, total=(b2 + (t3 - t2) * plan["reg_nc"][2]) * 64)


Units = collections.namedtuple("Units", "sub block qpos s0 s1 slot0 totals")


def units_of(plan):
    """Every 64-item block of every sub-queue, decoded as fetch_pixel decodes it (tile = queue position: a tile order only renames the
    tiles): arrays of the sub-queue, the block's number in it, the queue position of its tile, its samples [s0, s1) and the bank slot of
    (tile, first sample, pixel 0); totals[sub] = the items of each sub-queue."""
    nc, ln, sh = plan["reg_nc"], plan["reg_len"], plan["sub_shift"]
    cols, totals = [], []
    for sub in range(1 << sh):
        sq = subq_layout(plan, sub)
        totals.append(sq["total"])
        u = np.arange(sq["total"] >> 6, dtype=np.int64)
        r = (u >= sq["b1"]).astype(np.int64) + (u >= sq["b2"])                     # the region of the block
        base_b, base_t = np.array([0, sq["b1"], sq["b2"]])[r], np.array([0, sq["t1"], sq["t2"]])[r]
        r_nc, r_len = np.array(nc, np.int64)[r], np.array(ln, np.int64)[r]
        v = u - base_b
        lt = v // r_nc
        chunk = v - lt * r_nc
        qpos = ((lt + base_t) << sh) + sub
        s0 = chunk * r_len
        s1 = np.minimum(s0 + r_len, plan["n_samples"])
        slot0 = np.where(plan["bank_len"] != 0, qpos * plan["n_chunks"] + chunk, qpos * plan["n_samples"] + s0) * 64
        cols.append((np.full(len(u), sub, np.int64), u, qpos, s0, s1, slot0))
    return Units(*[np.concatenate(c) for c in zip(*cols)], totals=totals)


def _once(starts, ends, size):
    """How often each of [0, size) lies in one of the ranges [starts[i], ends[i])."""
    d = np.zeros(size + 1, np.int64)
    np.add.at(d, starts, 1)
    np.add.at(d, ends, -1)
    return np.cumsum(d)[:-1]


def assert_partition(plan):
    """The queue hands out every sample of every tile exactly once, and every bank slot exactly once."""
    u = units_of(plan)
    n_tiles, n = plan["n_tiles"], plan["n_samples"]
    assert sum(u.totals) == plan["total_work"], (u.totals, plan)
    assert all(t % 64 == 0 for t in u.totals)
    assert len(u.qpos) and (u.qpos >= 0).all() and (u.qpos < n_tiles).all(), plan                     # every queue position is a tile
    assert (u.s1 > u.s0).all() and (u.s0 >= 0).all() and (u.s1 <= n).all(), plan                      # no unit is empty
    seen = _once(u.qpos * n + u.s0, u.qpos * n + u.s1, n_tiles * n)
    assert (seen == 1).all(), (plan, np.flatnonzero(seen != 1)[:8])                                   # every (queue position, sample) once
    per_tile = plan["n_chunks"] if plan["bank_len"] else n
    held = 1 if plan["bank_len"] else u.s1 - u.s0                                                     # 64-slot rows a unit writes
    assert (u.slot0 % 64 == 0).all()
    rows = _once(u.slot0 // 64, u.slot0 // 64 + held, n_tiles * per_tile)
    assert (rows == 1).all(), (plan, np.flatnonzero(rows != 1)[:8])                                   # slot ranges disjoint, bank filled


def partition_key(plan):
    """What assert_partition reads of a plan: plans equal in this are the same partition."""
    return (plan["n_tiles"], plan["n_samples"], plan["n_chunks"], plan["bank_len"], plan["reg_q1"], plan["reg_q2"], tuple(plan["reg_len"]),
            tuple(plan["reg_nc"]), plan["sub_shift"], plan["total_work"])


# ---- frames, builds, cases ----------------------------------------------------------------------------------------------------------------
# name -> (width, height): the smallest frames that still reach the edge
FRAMES = {
    "t63": (72, 56),          # 9 x 7 tiles: one below the sub-queue threshold
    "t64": (64, 64),          # 8 x 8: at it
    "t65": (104, 40),         # 13 x 5: one above, 65 % 8 == 1
    "ragged81": (70, 67),     # 9 x 9: padding items in the last tile column and row, 81 % 8 == 1
    "wide": (128, 64),        # 128 tiles: enough work for explicit grids
    "banded": (64, 136),      # 8 x 17: bands of 64, 64 and 8 tiles
}


def tiles_of(frame, rows=None):
    w, h = FRAMES[frame]
    return cdiv(w, 8), cdiv(h if rows is None else rows, 8)


# kind -> (accel, flags that select it): the three sizes of workgroup a render of the common configuration runs in
BUILD_KINDS = {"brute": (R.ACCEL_BRUTE, 0), "bvh256": (R.ACCEL_BVH, R.FLAG_GLOBAL_NODES), "bvh768": (R.ACCEL_BVH, 0)}
GENERIC = R.FLAG_CPP_DIFFUSE       # a flag no folded build serves: the generic kernel (SPEC 0)


def build_tag(kind, flags=0):
    """The build of builds_common a render of `kind` with these flags runs: the common configuration's (SPEC 1), the one that folds
    RTW_FLAG_CHUNK_SUMS in (SPEC 3), the generic one (SPEC 0) under a reference-order flag."""
    spec = 0 if flags & GENERIC else (3 if flags & R.FLAG_CHUNK_SUMS else 1)
    if kind == "brute":
        return B.brute(0, spec, 0)
    if kind == "bvh256":
        return B.bvh(0, 0, spec, 0)
    return B.bvh(0, 1, spec, 0) if spec else None          # (the generic build has no large-workgroup form: render_choice says which it is)


@functools.lru_cache(maxsize=None)
def _tree_facts():
    from tests.test_bvh_builder_cpu import dump
    d = dump(R.Scene.generate(R.SCENE_C2))
    return len(d["nodes"]), d["depth"]


def build_choice(kind, flags=0):
    """rtw_render_choice for a render of the suite's Book-1 scene by `kind` with `flags`: {"build", "block", ..} as compiled today."""
    accel, kind_flags = BUILD_KINDS[kind]
    n_nodes, depth = _tree_facts()
    f = R.RtwRenderFacts(integrator=R.INTEGRATOR_GRADIENT, sampler=R.SAMPLER_ROW, depth=DEPTH, flags=flags | kind_flags)
    t = R.RtwTreeFacts(n_nodes=n_nodes, depth=depth, n_spheres=485, has_f16=1, has_planes=1)
    return R.render_choice(f, t, accel=accel)


# What a plan must show for a case to be the case it is named for
PROPERTIES = {
    "subq8": lambda q: q["sub_shift"] == 3,
    "single": lambda q: q["sub_shift"] == 0,
    "tiles>=64": lambda q: q["n_tiles"] >= 64,
    "tiles<64": lambda q: q["n_tiles"] < 64,
    "grid>=64": lambda q: q["grid"] >= 64,
    "grid<64": lambda q: q["grid"] < 64,
    "tiles%8": lambda q: q["n_tiles"] % 8 != 0,
    "one region": lambda q: q["reg_q1"] == q["reg_q2"] == q["n_tiles"],
    "region2": lambda q: q["reg_q1"] < q["reg_q2"],
    "region2 empty": lambda q: q["reg_q1"] == q["reg_q2"] < q["n_tiles"],
    "region3": lambda q: q["reg_q2"] < q["n_tiles"],
    "both capped": lambda q: q["n_tiles"] - q["reg_q2"] == q["reg_q2"] - q["reg_q1"] == q["n_tiles"] // 4,
    "bounds%8": lambda q: q["reg_q1"] % 8 != 0 and q["reg_q2"] % 8 != 0,
    "ragged r1": lambda q: q["n_samples"] % q["reg_len"][0] != 0,
    "ragged r2": lambda q: q["n_samples"] % q["reg_len"][1] != 0,
    "L2=1": lambda q: q["reg_len"][1] == 1,
    "L2=2": lambda q: q["reg_len"][1] == 2,
    "L2=4": lambda q: q["reg_len"][1] == 4,
    "grab 1": lambda q: q["grab_max"] == 64,
    "grab 2": lambda q: q["grab_max"] == 128,
    "grab 5": lambda q: q["grab_max"] == 320,
    "grab tile": lambda q: q["grab_max"] == 64 * q["n_chunks"],
    "13 blocks": lambda q: q["n_chunks"] == 13,
    "tile order": lambda q: q["has_tile_order"] == 1,
    "sums": lambda q: q["bank_len"] == 1 and q["chunk_len"] == SUM_CHUNK and q["reg_q1"] == q["reg_q2"] == q["n_tiles"],
    "ragged sum": lambda q: q["n_samples"] % SUM_CHUNK != 0,
    "block 256": lambda q: q["block"] == 256,
    "block 768": lambda q: q["block"] == 768,
}

# id: unique; frame, spp: the render; kind, flags: the build (BUILD_KINDS) and RtwParams.flags on top of the kind's; opts: the options set
# (everything else at its default); shows: per band, the PROPERTIES its plan must have; partition: (row_block, part_count) -- every
# part_index is rendered and the parts are put together --; band_rows: tile rows per band (RTW_OPT_SAMPLE_BANK_GB is set for it)
Case = collections.namedtuple("Case", "id group frame spp kind flags opts shows partition band_rows")


def case(id, group, frame, spp, kind, opts, shows, flags=0, partition=None, band_rows=None):
    shows = tuple(shows)
    if shows and not isinstance(shows[0], tuple):
        shows = (shows,)
    return Case(id, group, frame, spp, kind, flags, dict(opts), shows, partition, band_rows)


def _region_shows(chunk, spp, k):
    """Case B on ragged81 (81 tiles, a 256-thread build: the grid is the cap, at least 102 - 13 x 9 workgroups): what each length shows.
    13 and 25 leave a ragged last chunk in region 1 unless the length divides -- 13 at 13 spp, 5 at 25 spp -- and in region 2 always
    (L2 = 4 or 2 divides neither); region 3's units are single samples and never ragged; a length of 5 has L2 = 1: no region 2."""
    s = ["region3", "tiles%8"]
    if spp % min(chunk, spp):
        s.append("ragged r1")
    if chunk == 5:
        s += ["region2 empty", "L2=1"]
    else:
        s += ["region2", "ragged r2", "L2=4" if chunk >= 12 else "L2=2"]
        if k == 64:
            s += ["both capped", "bounds%8"]
    return s


def _cases():
    C, Q, T, G, S, O_, P = R.OPT_CHUNK_LEN, R.OPT_SUB_QUEUES, R.OPT_TAIL_UNITS, R.OPT_GRAB_BLOCKS, R.OPT_SAMPLE_BANK_GB, R.OPT_TILE_ORDER, R.OPT_BLOCKS_PER_CU
    out = []
    # A. the sub-queue threshold: 63 / 64 / 65 / 81 tiles, and 48 / 64 workgroups on 64 tiles
    for frame, big in (("t63", False), ("t64", True), ("t65", True), ("ragged81", True)):
        for sq in (0, 1):
            eight = big and sq == 0
            shows = ["subq8" if eight else "single", "tiles>=64" if big else "tiles<64", "grid>=64", "block 256"]
            if frame in ("t65", "ragged81"): shows.append("tiles%8")
            out.append(case(f"A-{frame}-sq{sq}", "A", frame, 25, "bvh256", {C: 6, Q: sq}, shows))
    out.append(case("A-t64-3chunks", "A", "t64", 12, "bvh256", {C: 4}, ["single", "tiles>=64", "grid<64", "block 256"]))       # 48 workgroups
    out.append(case("A-t64-4chunks", "A", "t64", 12, "bvh256", {C: 3}, ["subq8", "tiles>=64", "grid>=64", "block 256"]))       # 64 workgroups
    # B. regions x sub-queues
    for k in (0.5, 2, 64):
        for sq in (0, 1):
            for chunk in (5, 6, 11, 12, 13):
                for spp in (13, 25):
                    # (13 spp in units of 11, 12 or 13 is 2 / 2 / 1 units per tile: 41 workgroups or fewer, a single queue whatever the option)
                    eight = sq == 0 and 81 * cdiv(spp, min(chunk, spp)) * 64 >= 64 * 256
                    out.append(case(f"B-k{k}-sq{sq}-L{chunk}-{spp}spp", "B", "ragged81", spp, "bvh256", {C: chunk, Q: sq, T: k},
                                    _region_shows(chunk, spp, k) + ["subq8" if eight else "single"]))
    # C. grabs: 13 blocks per tile, so a grab of 2 or 5 crosses tile and region boundaries
    for blocks, name in ((0, "grab tile"), (1, "grab 1"), (2, "grab 2"), (5, "grab 5")):
        for sq in (0, 1):
            for k in (0, 2):
                out.append(case(f"C-g{blocks}-sq{sq}-k{k}", "C", "ragged81", 25, "bvh256", {C: 2, Q: sq, T: k, G: blocks},
                                [name, "13 blocks", "subq8" if sq == 0 else "single", "region3" if k else "one region"]))
    # D. tile orders
    for mode in (1, 2, 3, 4, 5):
        out.append(case(f"D-order{mode}", "D", "ragged81", 25, "bvh256", {C: 6, T: 2, O_: mode}, ["tile order", "subq8", "region2", "region3"]))
    # E. the three sizes of workgroup
    for kind in ("brute", "bvh256"):
        for frame in ("t65", "ragged81"):
            out.append(case(f"E-{kind}-{frame}", "E", frame, 25, kind, {C: 6}, ["subq8", "tiles%8", "block 256"]))
        out.append(case(f"E-{kind}-regions", "E", "ragged81", 25, kind, {C: 6, T: 2}, ["subq8", "region2", "region3", "bounds%8", "block 256"]))
    out.append(case("E-bvh768-t65", "E", "t65", 24, "bvh768", {C: 2}, ["subq8", "grid>=64", "tiles%8", "block 768"]))           # 65 workgroups
    out.append(case("E-bvh768-ragged81", "E", "ragged81", 20, "bvh768", {C: 2}, ["subq8", "grid>=64", "tiles%8", "block 768"])) # 68 workgroups
    out.append(case("E-bvh768-regions", "E", "ragged81", 57, "bvh768", {C: 6, T: 2},
                    ["subq8", "grid>=64", "region2", "region3", "ragged r1", "ragged r2", "bounds%8", "block 768"]))            # 68 workgroups
    out.append(case("E-bvh768-single", "E", "ragged81", 25, "bvh768", {C: 6}, ["single", "grid<64", "tiles>=64", "block 768"])) # 34 workgroups
    # G. bands of one render with and without sub-queues.  8 spp as the table says: the unit length the library picks is 2, a band of 64
    # tiles is 64 workgroups of 256 threads -- the 256-thread tree build, so that spp need not be raised.
    for name, opts in (("tail2", {T: 2}), ("order3", {O_: 3})):
        first = ["subq8", "tiles>=64", "grid>=64"] + (["region3", "region2 empty"] if name == "tail2" else ["tile order"])
        last = ["single", "tiles<64"] + (["region3"] if name == "tail2" else ["tile order"])
        out.append(case(f"G-{name}", "G", "banded", 8, "bvh256", opts, (tuple(first), tuple(first), tuple(last)), band_rows=8))
    # H. row partitions: three parts of ragged81 are 18 .. 36 tiles each -- single queues, and still right
    for rb in (1, 3, 8, 16):
        out.append(case(f"H-rb{rb}", "H", "ragged81", 25, "bvh256", {C: 6, T: 2}, ["single", "tiles<64", "region3"], partition=(rb, 3)))
    # ... and blocks of 3 rows dealt to two parts of the tall frame: 72 and 64 tiles, eight sub-queues under a partition
    out.append(case("H-rb3-subq8", "H", "banded", 25, "bvh256", {C: 6, T: 2}, ["subq8", "region2", "region3"], partition=(3, 2)))
    # I. chunk sums: one slot per unit, the regions off whatever RTW_OPT_TAIL_UNITS says, RTW_OPT_CHUNK_LEN ignored
    for frame in ("t65", "ragged81"):
        for spp in (13, 25):
            for sq in (0, 1):
                for gen in (0, GENERIC):
                    # 13 spp are 4 units per tile: 65 / 81 workgroups of 256 threads
                    out.append(case(f"I-{frame}-{spp}spp-sq{sq}-{'generic' if gen else 'folded'}", "I", frame, spp, "bvh256", {C: 7, T: 2, Q: sq},
                                    ["sums", "ragged sum", "subq8" if sq == 0 else "single", "tiles%8"], flags=R.FLAG_CHUNK_SUMS | gen))
    out.append(case("I-banded", "I", "banded", 13, "bvh256", {C: 7, T: 2}, (("sums", "subq8"), ("sums", "subq8"), ("sums", "single")),
                    flags=R.FLAG_CHUNK_SUMS, band_rows=8))
    out.append(case("I-parts", "I", "ragged81", 25, "bvh256", {C: 7, T: 2}, ["sums", "single"], flags=R.FLAG_CHUNK_SUMS, partition=(3, 3)))
    out.append(case("I-brute-generic", "I", "ragged81", 13, "brute", {T: 2}, ["sums", "subq8"], flags=R.FLAG_CHUNK_SUMS | GENERIC))
    out.append(case("I-bvh768", "I", "ragged81", 13, "bvh768", {T: 2}, ["sums", "single", "block 768"], flags=R.FLAG_CHUNK_SUMS))
    return out


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)
# F. explicit grids: RTW_OPT_BLOCKS_PER_CU 1, 2, 3, 6, 8, then 0 again, on `wide` at 64 spp in units of one sample (8192 blocks)
GRID_VALUES = (1, 2, 3, 6, 8, 0)
GRID_FRAME, GRID_SPP = "wide", 64


def by_group(group):
    return [c for c in CASES if c.group == group]


def part_rows(height, row_block, part_index, part_count):
    """The image rows of a partition, in the order of its compact rows."""
    return [j for j in range(height) if (j // row_block) % part_count == part_index]


def case_bands(c, part_index=0):
    """[(k_base, k_end, n_tiles)] of the bands a case's render (of one part) is launched in."""
    w, h = FRAMES[c.frame]
    rows = len(part_rows(h, c.partition[0], part_index, c.partition[1])) if c.partition else h
    tiles_x, tile_rows = cdiv(w, 8), cdiv(rows, 8)
    step = c.band_rows or max(tile_rows, 1)
    return [(t * 8, min((t + step) * 8, rows), tiles_x * (min(t + step, tile_rows) - t)) for t in range(0, tile_rows, step)]


def case_plans(c, n_cu=MI355X_CUS, block=None, part_index=0):
    """expected_plan for every band of a case (of one part), with the block its build compiles to today unless one is given."""
    flags = c.flags | BUILD_KINDS[c.kind][1]
    block = block or build_choice(c.kind, c.flags)["block"]
    sums = bool(flags & R.FLAG_CHUNK_SUMS)
    bands = case_bands(c, part_index)
    frame_tiles = sum(b[2] for b in bands)
    plans = []
    for k_base, k_end, n_tiles in bands:
        _, n_chunks = unit_length(c.spp, c.opts.get(R.OPT_CHUNK_LEN, 0), sums, frame_tiles, n_cu)
        grid = device_grid(n_cu, block, n_tiles, n_chunks, c.opts.get(R.OPT_BLOCKS_PER_CU, 0))
        q = expected_plan(n_tiles, c.spp, c.opts.get(R.OPT_CHUNK_LEN, 0), c.opts.get(R.OPT_TAIL_UNITS, 0.0), grid, block,
                          c.opts.get(R.OPT_SUB_QUEUES, 0), c.opts.get(R.OPT_GRAB_BLOCKS, 2), sums, frame_tiles, n_cu)
        mode = c.opts.get(R.OPT_TILE_ORDER, 0)
        q.update(bands=len(bands), tiles_x=cdiv(FRAMES[c.frame][0], 8), k_base=k_base, k_end=k_end,
                 has_tile_order=1 if mode and n_tiles > 2 else 0,                       # (modes 2 and 5 fall back to raster for quads / instances: none here)
                 row_block=c.partition[0] if c.partition else 8, part_index=part_index, part_count=c.partition[1] if c.partition else 1)
        plans.append(q)
    return plans


def assert_shows(c, plans):
    assert len(plans) == len(c.shows) or len(c.shows) == 1, (c.id, len(plans))
    for b, q in enumerate(plans):
        for name in c.shows[b if len(c.shows) > 1 else 0]:
            assert PROPERTIES[name](q), (c.id, b, name, q)


# ---- frames of the oracle, poison ------------------------------------------------------------------------------------------------------------
def view(frame, spp, flags=0):
    """(scene, camera, params) of a frame: the suite's small view of Book-1's final scene, gamma 1, depth 6."""
    w, h = FRAMES[frame]
    scene, cam, p = small_view(R.SCENE_C2, w, h, spp)
    p.gamma, p.depth, p.flags = 1.0, DEPTH, flags
    return scene, cam, p


def poison_seed(p):
    return (p.seed ^ POISON_SEED) & 0xFFFFFFFFFFFFFFFF


@functools.lru_cache(maxsize=None)
def _oracle(frame, spp, flags, poisoned):
    scene, cam, p = view(frame, spp, flags)
    if poisoned:
        p.seed = poison_seed(p)
    img, st = O.render(cam, scene, p, THREADS)
    img.setflags(write=False)
    return img, st


def oracle(frame, spp, flags=0):
    """(frame, RtwStats) of the CPU oracle, once per process, read-only.  Only the flags that define the image reach it."""
    return _oracle(frame, spp, flags & (R.FLAG_CHUNK_SUMS | GENERIC), False)


def oracle_poison(frame, spp, flags=0):
    return _oracle(frame, spp, flags & (R.FLAG_CHUNK_SUMS | GENERIC), True)


@functools.lru_cache(maxsize=None)
def _background(frame, spp, flags):
    """The frame of the same camera, seed and sampler over no scene at all: a pixel whose every camera ray misses everything has these bits."""
    scene, cam, p = view(frame, spp, flags)
    empty = R.Scene((), background=tuple(scene.pod.background))
    img, _ = O.render(cam, empty, p, THREADS)
    return img


def poison_differs(frame, spp, flags=0):
    """The share of the pixels that are not pure background in which the poison frame differs from the expected one (oracle, CPU)."""
    flags &= R.FLAG_CHUNK_SUMS | GENERIC
    want, bad = oracle(frame, spp, flags)[0], oracle_poison(frame, spp, flags)[0]
    lit = (want.view(np.uint32) != _background(frame, spp, flags).view(np.uint32)).any(axis=2)
    assert lit.mean() > 0.25, (frame, lit.mean())                      # the frame looks at the scene
    return float((want.view(np.uint32) != bad.view(np.uint32)).any(axis=2)[lit].mean())


def poison(renderer, cam, params):
    """Render the same frame under the same options with another seed and return its image: what the bank and the output buffer hold when
    the render under test begins is then wrong almost everywhere (poison_differs)."""
    q = R.RtwParams.from_buffer_copy(params)
    q.seed = poison_seed(params)
    img, _ = renderer.render(cam, q)
    return img
