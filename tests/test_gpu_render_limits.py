"""Renders at the limits the ABI declares, against the CPU oracle bit for bit.

A: frames 65535 wide, 65535 tall, and the far corner of a 65535 x 65535 frame through the row partition -- the shapes at which
`column | row << 16`, the 32-bit pixel id and the 32-bit bank slot of the render kernels (rtw_kernels.hip Pixel, fetch_pixel, resolve_kernel)
use every bit they have -- through the brute build and the three kinds of tree build, and over three contexts of one GPU (rtw_mgpu: the strided
2-D copy with rows of 786 420 bytes).  B: 2^24 - 1 samples in one pixel (`sample | samples left << 24`), the largest root of the stratified
and the fixed-centre samplers, the refusals one past each, and units of 255 samples.

Every shape is one rtw.h declares legal; the cases and their oracle frames live in render_limits_common.py (computed once, shared)."""
import numpy as np
import pytest

import rtw_amd as R
from tests import render_limits_common as X

pytestmark = pytest.mark.gpu

DEFAULTS = ((R.OPT_LIST_WALK_MAX, 48), (R.OPT_NODE_FORMAT, 0), (R.OPT_CHUNK_LEN, 0), (R.OPT_SAMPLE_BANK_GB, 48), (R.OPT_TILE_ORDER, 0),
            (R.OPT_TAIL_UNITS, 0))


@pytest.fixture(scope="module")
def ctx(rtw):
    """A context of this module's own for A: the options set here never reach another test."""
    with rtw.Renderer(0) as r:
        r.set_scene(X.book1())
        yield r


@pytest.fixture(scope="module")
def big(rtw):
    """One context for all of B, so that the bank of 2^24 - 1 samples is reserved once."""
    with rtw.Renderer(0) as r:
        yield r


def restore(r):
    for key, value in DEFAULTS:
        r.set_option(key, value)


def copy_params(p, **kw):
    q = R.RtwParams.from_buffer_copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def assert_frame(img, st, ref, st_ref, what):
    assert img.shape == ref.shape and img.tobytes() == ref.tobytes(), (what, int((img != ref).any(axis=-1).sum()), "pixels differ")
    for k in ("camera_rays", "segments", "rows"):
        assert getattr(st, k) == getattr(st_ref, k), (what, k, getattr(st, k), getattr(st_ref, k))
    assert st.nan_pixels == 0, (what, st.nan_pixels)


def through_builds(r, name, options=(), device_out=False, what=None):
    """Render frame `name` through the four builds of X.BUILDS under `options`, each asserted by name and against the oracle; -> the frames."""
    cam, p = X.frame_case(name)
    ref, st_ref = X.frame_oracle(name)
    frames = []
    try:
        for key, value in options:
            r.set_option(key, value)
        r.set_option(R.OPT_LIST_WALK_MAX, 0)
        for build, accel, node_format, flags in X.BUILDS:
            r.set_option(R.OPT_NODE_FORMAT, node_format)
            q = copy_params(p, accel=accel, flags=p.flags | flags)
            if device_out:
                import torch
                t = torch.full(ref.shape, -7.5, dtype=torch.float32, device="cuda:0")
                torch.cuda.synchronize()
                _, st = r.render(cam, q, out=t.data_ptr())
                img = t.cpu().numpy()
            else:
                img, st = r.render(cam, q)
            got = r.last_render_build()
            assert got.startswith(build), (name, what, build, got)
            assert_frame(img, st, ref, st_ref, (name, what, build))
            frames.append(img)
    finally:
        restore(r)
    return frames


# ---- A: frame shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["65535x1", "65534x1"])
@pytest.mark.parametrize("device_out", [False, True])
def test_widest_frame(ctx, name, device_out):
    """8192 tiles in one tile row, seven of the eight rows of every tile padding; into host memory and into a torch tensor."""
    through_builds(ctx, name, device_out=device_out)


def test_tallest_frame(ctx):
    """One tile column, 8192 tile rows, in one band."""
    through_builds(ctx, "1x65535")


def test_tallest_frame_in_bands(ctx):
    """... and in 82 bands of 100 tile rows, the last of 92 (test_render_limits_cpu.py checks the budget's arithmetic)."""
    through_builds(ctx, "1x65535", options=((R.OPT_SAMPLE_BANK_GB, X.bank_gb_for_band(1, 1, 100)),), what="bands")


def test_corner_row(ctx, rtw):
    """row_block 1, partition 65534 of 65535: image row 65534 of a 65535 x 65535 frame alone."""
    assert rtw.lib().rtw_part_rows(X.DIM_MAX, 1, X.DIM_MAX - 1, X.DIM_MAX) == 1
    assert through_builds(ctx, "corner row")[0].shape == (1, X.DIM_MAX, 3)


@pytest.mark.parametrize("tile_order", [0, 1, 2, 3])
def test_corner_block(ctx, rtw, tile_order):
    """row_block 8, partition 8191 of 8192: the ragged last block, rows 65528 .. 65534, in every tile order."""
    assert rtw.lib().rtw_part_rows(X.DIM_MAX, 8, 8191, 8192) == 7
    frames = through_builds(ctx, "corner block", options=((R.OPT_TILE_ORDER, tile_order),), what=f"tile order {tile_order}")
    assert frames[0].shape == (7, X.DIM_MAX, 3)


def test_corner_block_guided_units(ctx):
    """... and with the queue's last tiles cut into units of one sample (RTW_OPT_TAIL_UNITS 2) at 6 spp in units of 6."""
    through_builds(ctx, "corner block 6spp", options=((R.OPT_TAIL_UNITS, 2), (R.OPT_CHUNK_LEN, 6)), what="tail units")


@pytest.mark.parametrize("row_block", [8, 5])
def test_wide_frame_over_three_contexts(ctx, rtw, row_block):
    """65535 x 24 over rtw_mgpu on three contexts of GPU 0, blocks of 8 rows and the ragged blocks of 5: staged into a pageable numpy frame,
    and by the strided 2-D copy (rows of 786 420 bytes, a pitch of three blocks) into a device tensor."""
    import torch
    name = "65535x24"
    cam, p = X.frame_case(name)
    ref, st_ref = X.frame_oracle(name)
    single = through_builds(ctx, name)[1]                             # (the automatic build's frame; through_builds has compared all four)
    with rtw.MultiRenderer([0, 0, 0]) as m:
        m.set_scene(X.book1())
        for accel in (R.ACCEL_BVH, R.ACCEL_BRUTE):
            q = copy_params(p, accel=accel, row_block=row_block)
            host = np.full(ref.shape, -7.5, np.float32)
            _, tot, per = m.render(cam, q, out=host)
            assert host.tobytes() == single.tobytes() == ref.tobytes(), (row_block, accel, "staged", int((host != ref).any(axis=-1).sum()))
            assert tot.segments == st_ref.segments == sum(s.segments for s in per) and tot.camera_rays == st_ref.camera_rays
            assert [s.rows for s in per] == [rtw.lib().rtw_part_rows(24, row_block, k, 3) for k in range(3)]
            t = torch.full(ref.shape, -7.5, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            _, tot, per = m.render(cam, q, out=t.data_ptr())
            dev = t.cpu().numpy()
            assert dev.tobytes() == single.tobytes() == ref.tobytes(), (row_block, accel, "2-D copy", int((dev != ref).any(axis=-1).sum()))
            assert tot.segments == st_ref.segments and tot.nan_pixels == 0


def test_one_past_the_limit_is_refused_and_the_context_renders_on(ctx):
    cam, p = X.frame_case("65535x1")
    for w, h in ((X.DIM_MAX + 1, 1), (1, X.DIM_MAX + 1)):
        with pytest.raises(R.RtwError) as e:
            ctx.render(cam, copy_params(p, width=w, height=h))
        assert e.value.status == X.E_INVALID, (w, h, e.value.status)
    through_builds(ctx, "65535x1", what="after the refusals")


# ---- B: sample counts -----------------------------------------------------------------------------------------------------------------
def render_pixel(big, integrator, sampler, samples, flags=0, background=(0.0, 0.0, 0.0)):
    big.set_scene(X.empty_scene(background))
    return big.render(X.pixel_camera(), X.pixel_params(integrator, sampler, samples, flags))


@pytest.mark.parametrize("integrator,sampler,samples,rays", X.SAMPLE_CASES)
def test_sample_count_limits(big, integrator, sampler, samples, rays):
    """A 1 x 1 frame of the empty scene: every path is a miss.  Without RTW_FLAG_CHUNK_SUMS the bank of its one tile at 2^24 - 1 samples
    is 64 x 12 B x 16 777 215 = 12.9 GB, about the bench frame's bank (12.4 GB).  Such a render takes 6.5 s on an MI355X (one lane of the
    resolve adds the pixel's 16.7 M slots in order); the count is the limit itself and is not shrunk."""
    if rays is None:
        with pytest.raises(R.RtwError) as e:
            render_pixel(big, integrator, sampler, samples)
        assert e.value.status == X.E_INVALID, e.value.status
        return
    ref, st_ref = X.pixel_oracle(integrator, sampler, samples)
    img, st = render_pixel(big, integrator, sampler, samples)
    print(f"sampler {sampler} samples {samples}: kernel {st.kernel_ms:.1f} ms, total {st.total_ms:.1f} ms, oracle {st_ref.total_ms:.1f} ms")
    assert st.camera_rays == rays == st_ref.camera_rays, (st.camera_rays, rays, st_ref.camera_rays)
    assert st.segments == st_ref.segments and st.nan_pixels == 0
    assert X.same_bits(img, ref), (img, ref)


def test_chunk_sums_at_the_largest_count(big):
    ref, st_ref = X.pixel_oracle(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW, X.SAMPLES_MAX, R.FLAG_CHUNK_SUMS)
    img, st = render_pixel(big, R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW, X.SAMPLES_MAX, R.FLAG_CHUNK_SUMS)
    print(f"chunk sums: kernel {st.kernel_ms:.1f} ms, total {st.total_ms:.1f} ms")
    assert st.camera_rays == X.SAMPLES_MAX == st_ref.camera_rays
    assert X.same_bits(img, ref), (img, ref)
    plain, _ = X.pixel_oracle(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW, X.SAMPLES_MAX)
    assert not X.same_bits(plain, ref), "the two associations agree at this count: the flag's sum is not pinned by it"


@pytest.mark.parametrize("flags", [0, R.FLAG_CHUNK_SUMS])
def test_sum_order_at_the_largest_count(big, flags):
    """16 777 215 samples of the background (3.0, 0.1, 1.0), against numpy alone: the in-order sum stalls at 2^24 (1.0), loses most of 0.1."""
    want = (X.mean_chunk_sums if flags else X.mean_in_order)(X.SUM_BIG_BACKGROUND, X.SAMPLES_MAX)
    img, st = render_pixel(big, R.INTEGRATOR_BG_COLOR, R.SAMPLER_ROW, X.SAMPLES_MAX, flags, X.SUM_BIG_BACKGROUND)
    print(f"flags {flags}: mean {img.ravel()} of {X.SUM_BIG_BACKGROUND}; kernel {st.kernel_ms:.1f} ms")
    assert st.camera_rays == X.SAMPLES_MAX and st.nan_pixels == 0
    assert X.same_bits(img.reshape(3), want), (img, want)
    assert not np.array_equal(want, np.float32(X.SUM_BIG_BACKGROUND))


@pytest.mark.parametrize("samples", [255, 256, 511])
def test_longest_unit(ctx, oracle, samples):
    """RTW_OPT_CHUNK_LEN 255, the most `samples left` holds: one whole unit, one and a unit of one, one and a ragged one, on a ragged 9 x 9."""
    cam, p = X.field_camera(9, 9), X.frame_params(9, 9, samples)
    ref, st_ref = oracle.render(cam, X.book1(), p, X.THREADS)
    try:
        ctx.set_option(R.OPT_CHUNK_LEN, 255)
        ctx.set_option(R.OPT_LIST_WALK_MAX, 0)
        for build, accel, node_format, flags in X.BUILDS:
            ctx.set_option(R.OPT_NODE_FORMAT, node_format)
            img, st = ctx.render(cam, copy_params(p, accel=accel, flags=flags))
            assert ctx.last_render_build().startswith(build), (build, ctx.last_render_build())
            assert st.camera_rays == 81 * samples
            assert_frame(img, st, ref, st_ref, (samples, build))
    finally:
        restore(ctx)
