"""What the a-trous tests share (tests/test_atrous_cpu.py, tests/test_gpu_atrous.py): the case matrix, its inputs, and a numpy
restatement of the rule of include/rtw.h ("a-trous filter").

The restatement is vectorised per tap, in tap order (dy outer, dx inner), over the pixels whose tap lies inside the frame; a tap of weight 0
is left out through np.where.  Every numpy operation on float32 arrays rounds once, so each pixel sees the host form's operation sequence,
with the library's own exp_plain (pinned by tests/test_guided_cpu.py).

Bit for bit here means: the same 32 bits, or a NaN on both sides.  The sign and payload of a NaN that an operation creates (inf - inf,
0 * inf) are the processor's choice -- x86 sets the sign bit, the GPU does not -- and no rule of the filter reads them."""
import functools

import numpy as np

import rtw_amd as R

F = np.float32
SHAPES = [(1, 1), (3, 5), (9, 17), (35, 67)]                # (h, w): frames 1 x 1, 5 x 3, 17 x 9 and 67 x 35
LEVELS = [1, 3, 8]                                          # at 8 the step (128) exceeds every frame of SHAPES: only the centre tap remains (DEEP_SHAPES)
SIGMA_COLOR, SIGMA_DEPTH, SIGMA_NORMAL, FLOOR = 0.75, 0.5, 0.6, 0.05
# name -> (sigma_color, sigma_depth, sigma_normal, same_object, albedo, emitted)
TERM_SETS = {
    "color": (SIGMA_COLOR, 0.0, 0.0, False, False, False),
    "depth": (0.0, SIGMA_DEPTH, 0.0, False, False, False),
    "normal": (0.0, 0.0, SIGMA_NORMAL, False, False, False),
    "idx": (0.0, 0.0, 0.0, True, False, False),
    "all": (SIGMA_COLOR, SIGMA_DEPTH, SIGMA_NORMAL, True, False, False),
    "all+albedo": (SIGMA_COLOR, SIGMA_DEPTH, SIGMA_NORMAL, True, True, False),
    "all+albedo+emitted": (SIGMA_COLOR, SIGMA_DEPTH, SIGMA_NORMAL, True, True, True),
    "none+emitted": (0.0, 0.0, 0.0, False, False, True),
}
# Levels 7 and 8 with taps inside the frame: 259 = 2 * 128 + 3 columns (or rows), so that at step 128 the taps at -256 .. +256 of some
# pixel all land inside.  The term sets are those whose weights stay positive that far away -- none has the colour term, whose sigma
# shrinks by 2^-i -- and the frame is deep_frame's: inputs' with its three non-finite pixels made finite, for without the colour term a
# NaN tap is not dropped and seven levels spread it over the whole strip, where every level count gives the same answer, NaN.
DEEP_SHAPES = [(3, 259), (259, 3)]
DEEP_LEVELS = [7, 8]
DEEP_TERM_SETS = {
    "depth": TERM_SETS["depth"],
    "normal": TERM_SETS["normal"],
    "none+emitted": TERM_SETS["none+emitted"],
    "guides+albedo+emitted": (0.0, SIGMA_DEPTH, SIGMA_NORMAL, False, True, True),
}


def same_bits(a, b):
    """The same bits, or NaN on both sides (module docstring)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def mismatch(a, b):
    bad = ~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))
    i = np.argwhere(bad)
    return f"{int(bad.sum())} of {bad.size} differ, first at {i[0].tolist()}: {a[tuple(i[0])]!r} != {b[tuple(i[0])]!r}" if len(i) else "equal"


@functools.lru_cache(maxsize=None)
def inputs(h, w, seed=5):
    """A noisy frame over three objects and a miss region, with every special the rule names: NaN and infinite pixels, a NaN depth, miss
    pixels (idx -1, normal 0 0 0, albedo 0 0 0, the far depth), albedo channels just below and exactly at the floor, emission on one object.
    Read-only arrays."""
    rng = np.random.default_rng(seed * 1000 + h * 131 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    ids = ((xx * 3) // max(w, 1) + ((yy * 2) // max(h, 1)) * 3).astype(np.int32) % 4 - 1          # -1 (miss), 0, 1, 2 in blocks
    miss = ids < 0
    depth = (4.0 + 0.05 * xx + 0.11 * yy + 3.0 * ids + 0.02 * rng.standard_normal((h, w))).astype(F)
    depth[miss] = F(1600.0)
    normal = rng.standard_normal((h, w, 3)).astype(F) * F(0.15) + np.eye(3, dtype=F)[np.clip(ids, 0, 2)]
    normal = (normal / np.sqrt((normal * normal).sum(-1, keepdims=True))).astype(F)
    normal[miss] = 0.0
    albedo = (0.2 + 0.7 * rng.random((h, w, 3))).astype(F)
    albedo[miss] = 0.0
    emitted = np.zeros((h, w, 3), F)
    emitted[ids == 2] = rng.random((int((ids == 2).sum()), 3)).astype(F) * F(2.0)
    frame = (albedo * (0.5 + 0.5 * rng.random((h, w, 3))) + emitted + np.where(miss[..., None], F(0.7), F(0.0))).astype(F)
    flat = lambda a: a.reshape(-1, a.shape[-1]) if a.ndim == 3 else a.reshape(-1)
    n = h * w
    if n >= 15:
        spots = rng.choice(n, 8, replace=False)
        flat(frame)[spots[0]] = np.nan                                   # a NaN pixel
        flat(frame)[spots[1], 1] = np.inf                                # an infinite channel
        flat(frame)[spots[2]] = (-np.inf, 1.0, np.nan)
        flat(depth)[spots[3]] = np.nan
        flat(albedo)[spots[4]] = (np.nextafter(F(FLOOR), F(0.0)), F(FLOOR), np.nextafter(F(FLOOR), F(1.0)))   # just below, at, just above
        flat(albedo)[spots[5]] = (F(FLOOR), 0.0, np.nextafter(F(FLOOR), F(0.0)))
        flat(frame)[spots[6]] = 40.0                                     # a firefly
        flat(normal)[spots[7]] = (np.nan, 0.0, 1.0)
    else:
        albedo[0, 0] = (np.nextafter(F(FLOOR), F(0.0)), F(FLOOR), 0.9)
    out = dict(frame=frame, depth=depth, normal=normal, ids=ids, albedo=albedo, emitted=emitted)
    for a in out.values():
        a.setflags(write=False)
    return out


def call_kwargs(h, w, terms, levels):
    """The keyword arguments of atrous_filter / Renderer.atrous_filter for one case (the frame is inputs(h, w)["frame"])."""
    sc, sd, sn, same, alb, emi = TERM_SETS[terms] if terms in TERM_SETS else DEEP_TERM_SETS[terms]
    g = inputs(h, w)
    return dict(depth=g["depth"] if sd > 0 else None, normal=g["normal"] if sn > 0 else None, ids=g["ids"] if same else None,
                albedo=g["albedo"] if alb else None, emitted=g["emitted"] if emi else None, levels=levels, sigma_color=sc,
                sigma_depth=sd, sigma_normal=sn, same_object=same, albedo_floor=FLOOR)


def _exp_plain(x):
    return R.exp_plain(np.ascontiguousarray(x, F).reshape(-1)).reshape(x.shape)


def ref_atrous(frame, depth=None, normal=None, ids=None, albedo=None, emitted=None, levels=5, sigma_color=0.0, sigma_depth=0.0,
               sigma_normal=0.0, same_object=False, albedo_floor=0.0):
    """The rule of include/rtw.h in numpy, float32 throughout (module docstring).  A guide that is None has its term off."""
    frame = np.asarray(frame, F)
    h, w, _ = frame.shape
    K = [F(0.375), F(0.25), F(0.0625)]
    sd = sigma_depth if depth is not None else 0.0
    sn = sigma_normal if normal is not None else 0.0
    same = same_object and ids is not None
    with np.errstate(all="ignore"):
        a = np.where(albedo >= F(albedo_floor), albedo, F(1.0)).astype(F) if albedo is not None else np.ones_like(frame)
        e = np.asarray(emitted, F) if emitted is not None else np.zeros_like(frame)
        c = (frame - e) / a
        inv_depth = F(0.5) / (F(sd) * F(sd)) if sd > 0 else F(0.0)
        inv_normal = F(0.5) / (F(sn) * F(sn)) if sn > 0 else F(0.0)
        for i in range(levels):
            s, scale = 1 << i, F(2.0 ** -i)
            sc_i = F(sigma_color) * scale
            inv_color = F(0.5) / (sc_i * sc_i) if sigma_color > 0 else F(0.0)
            total, wsum = np.zeros((h, w, 3), F), np.zeros((h, w), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    y0, y1, x0, x1 = max(0, -dy * s), min(h, h - dy * s), max(0, -dx * s), min(w, w - dx * s)
                    if y0 >= y1 or x0 >= x1:
                        continue                                          # the tap is outside the frame for every pixel
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))
                    hw = K[abs(dx)] * K[abs(dy)]
                    acc = np.zeros((y1 - y0, x1 - x0), F)
                    if sigma_color > 0:
                        d = c[Q] - c[P]
                        acc = acc + inv_color * ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
                    if sd > 0:
                        dz = (depth[Q] - depth[P]) * scale
                        acc = acc + inv_depth * (dz * dz)
                    if sn > 0:
                        d = normal[Q] - normal[P]
                        acc = acc + inv_normal * ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
                    g = np.where(acc >= 0, _exp_plain(-acc), F(0.0)).astype(F)
                    if same:
                        g = np.where(ids[Q] != ids[P], F(0.0), g)
                    wt = hw * g
                    take = wt > 0
                    total[P] = np.where(take[..., None], total[P] + c[Q] * wt[..., None], total[P])
                    wsum[P] = np.where(take, wsum[P] + wt, wsum[P])
            c = np.where((wsum > 0)[..., None], total / wsum[..., None], c).astype(F)
        return (c * a + e).astype(F)


@functools.lru_cache(maxsize=None)
def host_answer(h, w, terms, levels):
    """The host form's answer of one case, computed once (read-only)."""
    out = R.atrous_filter(inputs(h, w)["frame"], **call_kwargs(h, w, terms, levels))[0]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def deep_frame(h, w):
    """inputs(h, w)'s frame with its non-finite pixels set to 0.5 (DEEP_SHAPES' comment).  Read-only."""
    frame = inputs(h, w)["frame"].copy()
    frame[~np.isfinite(frame).all(-1)] = 0.5
    frame.setflags(write=False)
    return frame


@functools.lru_cache(maxsize=None)
def deep_answer(h, w, terms, levels):
    """The host form's (answer, taps) on deep_frame, computed once (read-only)."""
    out, st = R.atrous_filter(deep_frame(h, w), **call_kwargs(h, w, terms, levels))
    out.setflags(write=False)
    return out, int(st.taps)


def taps_inside(h, w, levels):
    """The taps inside an h x w frame over `levels` levels, and the count were every level left with its centre tap alone."""
    taps = sum(sum(max(0, w - abs(d) * 2 ** i) for d in range(-2, 3)) * sum(max(0, h - abs(d) * 2 ** i) for d in range(-2, 3)) for i in range(levels))
    return taps, levels * h * w
