"""What the bloom tests share (tests/test_bloom_cpu.py, tests/test_gpu_bloom.py): the rule of include/rtw.h "bloom" restated in numpy, and the
frames it is run on.

  * restate_bloom(frame, T=float32): operation by operation -- every numpy operation on float32 arrays rounds once, as every written
    operation of csrc/rtw_bloom.h does under -ffp-contract=off; the sums take their taps in the rule's order (rows outer, columns inner), a
    skipped tap leaves sum and wsum as they were.
  * restate_bloom(frame, T=float64): the same text in float64; the float32 constants of the rule (0.2126f ...) and the call's parameters enter
    as the float32 values they are, since they are the rule's data and no rounding of the arithmetic.
  * bloom_bound: the float64 run again with a second field E beside every value V, the bound on |float32 - float64| of that value.

The float64 bound.  u = 2^-24; channels in [0, 2^8] that are 0 or far above the subnormals, so every sum is of non-negative terms and only
Y - threshold cancels.  A sum's relative error is its worst operand's plus u, a product's or quotient's the sum of its operands' plus u.
  bright pass   Y: products 1, the sums 2, 3:  3 u.   s = Y - threshold:  |ds| <= 3 u Y + u |s| <= 4 u M,  M = max(Y, threshold).
                c outside the knee is max(s, 0): dc <= ds.  Inside, q = s + knee (dq <= ds + u q), c = q q / (4 knee): the square u, 4 knee
                exact, the divide u:  dc <= 2 (dq / q) c + 2 u c = ds q / (2 knee) + 4 u c <= ds + 4 u c  as q <= 2 knee.  The two pieces meet
                with equal value and slope at both ends, so a side that takes the other piece is within the same ds.   dc <= 4 u M + 4 u c.
                k = c / Y:  dk <= dc / Y + (3 + 1) u k.   b = x k:  db <= x dk + u b = 4 u M x / Y + 9 u b           =: e_b (per channel)
                kw = 1 / (1 + L), L = luma(b):  dL <= luma(e_b) + 3 u L;  1 + L: + u (1 + L);  relative to 1 + L >= 1 that is at most
                luma(e_b) + 4 u;  the divide u.   wt = (D / 128) kw: one more.          eps = luma(e_b) + 6 u  (0 without Karis: kw = 1)
  down          out = N / W,  N = sum wt v,  W = sum wt.  Errors e of the values move out by at most their average under the same weights;
                relative errors eps of the weights move N and W by at most eps each, out by 2 eps;  the products u, at most 36 additions,
                36 u:  N 37 u;  W 36 u in the first step and exact afterwards (the weights are multiples of 1 / 128 that sum to at most 1);
                the divide u.      E' = avg(E) + V' (2 eps_max + 74 u)  in the first step (eps_max over the whole frame),
                                   E' = avg(E) + 38 u V'                afterwards
  U             16 taps, dyadic weights: N 17 u, W exact, the divide u:                  E_U = avg(E) + 18 u U
  up            level + spread * U: the product u, the sum u:                            E' = E_l + spread E_U + u spread U + u V'
  composite     in + intensity * B likewise:                                             E_out = intensity E_B + u intensity B + u out
and the layer's bound is E_B.  Everything times 1.01 for the second-order terms."""
import numpy as np

import rtw_amd as R

F = np.float32
U = 2.0 ** -24
SIZES = [(1, 1), (2, 2), (3, 3), (5, 3), (33, 33), (65, 35), (64, 48), (257, 3)]
SIZE_IDS = lambda s: f"{s[0]}x{s[1]}"
D = np.array([[1, 1, 2, 2, 1, 1], [1, 5, 6, 6, 5, 1], [2, 6, 8, 8, 6, 2], [2, 6, 8, 8, 6, 2], [1, 5, 6, 6, 5, 1], [1, 1, 2, 2, 1, 1]])
UP = {1: (3, 7, 5, 1), 3: (1, 5, 7, 3)}
# karis x (threshold, knee): no knee, knee == threshold, threshold 0, an ordinary one
PARAM_SETS = [dict(karis=k, threshold=t, knee=n) for k in (False, True) for t, n in ((1.0, 0.0), (0.75, 0.75), (0.0, 0.0), (1.0, 0.5))]


def same_bits(a, b):
    """The same bits, or (float32) NaN on both sides."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def noise(w, h, seed=0, top=256.0):
    """A linear frame over 22 stops up to `top`: 2^uniform(-14, log2 top), a few exact zeros, a few emitters at 40 times their surroundings."""
    rng = np.random.default_rng(1000 * w + h + seed)
    f = np.exp2(rng.uniform(-14.0, np.log2(top) - 6.0, (h, w, 3)))
    hot = rng.random((h, w)) < 0.1
    f[hot] *= 40.0
    f[rng.random((h, w)) < 0.05] = 0.0
    return f.astype(F)


def special_frame(w=9, h=7):
    """noise with one NaN pixel, one +inf, one -inf (each in one channel) and one negative channel."""
    f = noise(w, h, seed=5)
    f[1, 2, 0] = np.nan
    f[3, 4, 1] = np.inf
    f[5, 6, 2] = -np.inf
    f[2, 7, 1] = -3.0
    return f


def levels_restated(w, h, levels):
    """The sizes of levels 1 .. n by the rule's text."""
    out = []
    while len(out) < levels:
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
        if (w, h) == (1, 1):
            break
    return out


def luma(x, T):
    return (T(F(0.2126)) * x[..., 0] + T(F(0.7152)) * x[..., 1]) + T(F(0.0722)) * x[..., 2]


def knee_curve(Y, threshold, knee, T):
    """c of the bright pass for luminances Y."""
    thr, kn = T(F(threshold)), T(F(knee))
    s = Y - thr
    with np.errstate(all="ignore"):
        quad = ((s + kn) * (s + kn)) / (T(4.0) * kn)
    return np.where((kn > 0) & (s > -kn) & (s < kn), quad, np.where(s > 0, s, T(0.0))).astype(T)


def bright(frame, threshold, knee, karis, T):
    """(b [h][w][3], kw [h][w]) of the bright pass; kw = -1 where the pixel is not usable."""
    x = frame.astype(T)
    usable = np.isfinite(x).all(-1)
    with np.errstate(all="ignore"):
        x = np.where(x < 0, T(0.0), x)
        Y = luma(x, T)
        c = knee_curve(Y, threshold, knee, T)
        b = np.where((Y > 0)[..., None], x * (c / Y)[..., None], T(0.0)).astype(T)
        kw = T(1.0) / (T(1.0) + luma(b, T)) if karis else np.ones(Y.shape, T)
    return np.where(usable[..., None], b, T(0.0)).astype(T), np.where(usable, kw, T(-1.0)).astype(T)


def down(fields, kw, T):
    """One down step of the fields [k][h][w][3] under the tap factors kw [h][w] (< 0: no tap): ([k][h'][w'][3], taps inside the level)."""
    k, h, w, _ = fields.shape
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    I, J = np.arange(w2), np.arange(h2)
    acc, wsum, taps = np.zeros((k, h2, w2, 3), T), np.zeros((h2, w2), T), 0
    with np.errstate(all="ignore"):
        for b in range(-2, 4):
            y = 2 * J + b
            my, yc = (y >= 0) & (y < h), np.clip(y, 0, h - 1)
            for a in range(-2, 4):
                x = 2 * I + a
                mx, xc = (x >= 0) & (x < w), np.clip(x, 0, w - 1)
                inside = my[:, None] & mx[None, :]
                taps += int(inside.sum())
                kwt = kw[yc][:, xc]
                use = inside & ~(kwt < 0)
                wt = (T(D[b + 2][a + 2]) / T(128.0)) * kwt
                v = fields[:, yc][:, :, xc]
                acc = np.where(use[None, :, :, None], acc + v * wt[None, :, :, None], acc)
                wsum = np.where(use, wsum + wt, wsum)
        out = np.where((wsum > 0)[None, :, :, None], acc / wsum[None, :, :, None], T(0.0))
    return out.astype(T), taps


def foot(n):
    """For fine coordinates 0 .. n - 1: the first of the four coarse coordinates and the four weights."""
    i = np.arange(n)
    N = 2 * i - 1
    I0 = N // 4                                                # floor division: -1 at i = 0
    r = N - 4 * I0
    assert set(r.tolist()) <= {1, 3}
    return I0 - 1, np.array([UP[int(q)] for q in r])


def up(fields, w, h, T):
    """U of the coarse fields [k][h'][w'][3] at every pixel of a w x h finer level: ([k][h][w][3], taps)."""
    k, hc, wc, _ = fields.shape
    x0, wx = foot(w)
    y0, wy = foot(h)
    acc, wsum, taps = np.zeros((k, h, w, 3), T), np.zeros((h, w), T), 0
    with np.errstate(all="ignore"):
        for ky in range(4):
            y = y0 + ky
            my, yc = (y >= 0) & (y < hc), np.clip(y, 0, hc - 1)
            for kx in range(4):
                x = x0 + kx
                mx, xc = (x >= 0) & (x < wc), np.clip(x, 0, wc - 1)
                inside = my[:, None] & mx[None, :]
                taps += int(inside.sum())
                wt = (wy[:, ky][:, None] * wx[:, kx][None, :]).astype(T) / T(256.0)
                v = fields[:, yc][:, :, xc]
                acc = np.where(inside[None, :, :, None], acc + v * wt[None, :, :, None], acc)
                wsum = np.where(inside, wsum + wt, wsum)
        assert (wsum > 0).all()
        out = acc / wsum[None, :, :, None]
    return out.astype(T), taps


def restate_bloom(frame, levels=6, threshold=1.0, knee=0.5, karis=True, spread=0.5, intensity=0.25, T=F):
    """(out, layer, taps, the levels 1 .. n after the way up) of the rule in T."""
    h, w, _ = frame.shape
    sizes = levels_restated(w, h, levels)
    b, kw = bright(frame, threshold, knee, karis, T)
    lv, taps = [], 0
    cur, t = down(b[None], kw, T)
    lv.append(cur)
    taps += t
    for _ in sizes[1:]:
        cur, t = down(cur, np.ones(cur.shape[1:3], T), T)
        lv.append(cur)
        taps += t
    assert [(a.shape[2], a.shape[1]) for a in lv] == sizes
    with np.errstate(all="ignore"):
        for l in range(len(lv) - 2, -1, -1):
            u, t = up(lv[l + 1], lv[l].shape[2], lv[l].shape[1], T)
            lv[l] = (lv[l] + T(F(spread)) * u).astype(T)
            taps += t
        layer, t = up(lv[0], w, h, T)
        taps += t
        out = (frame.astype(T) + T(F(intensity)) * layer[0]).astype(T)
    return out, layer[0], taps, [a[0] for a in lv]


def bloom_bound(frame, levels=6, threshold=1.0, knee=0.5, karis=True, spread=0.5, intensity=0.25):
    """(out64, layer64, bound_out, bound_layer): the rule in float64 and, per value, the bound on what float32 arithmetic may differ by (the
    module docstring derives it).  frame: finite, channels 0 or well above the subnormals."""
    T = np.float64
    assert np.isfinite(frame).all() and (frame >= 0).all()
    h, w, _ = frame.shape
    sizes = levels_restated(w, h, levels)
    x = frame.astype(T)
    b, kw = bright(frame, threshold, knee, karis, T)
    Y = luma(x, T)
    M = np.maximum(Y, float(F(threshold)))
    with np.errstate(all="ignore"):
        ratio = np.where((Y > 0)[..., None], x / Y[..., None], 0.0)
    e_b = 4 * U * M[..., None] * ratio + 9 * U * b
    eps = float((luma(e_b, T) + 6 * U).max()) if karis else 0.0
    both, _ = down(np.stack([b, e_b]), kw, T)
    V, E = both[0], both[1] + both[0] * (2 * eps + 74 * U)
    lv = [(V, E)]
    for _ in sizes[1:]:
        both, _ = down(np.stack([V, E]), np.ones(V.shape[:2], T), T)
        V, E = both[0], both[1] + 38 * U * both[0]
        lv.append((V, E))
    sp, it = float(F(spread)), float(F(intensity))

    def u_of(l, fw, fh):
        both, _ = up(np.stack(lv[l]), fw, fh, T)
        return both[0], both[1] + 18 * U * both[0]

    for l in range(len(lv) - 2, -1, -1):
        Uv, Ue = u_of(l + 1, lv[l][0].shape[1], lv[l][0].shape[0])
        V = lv[l][0] + sp * Uv
        lv[l] = (V, lv[l][1] + sp * Ue + U * sp * Uv + U * V)
    B, Be = u_of(0, w, h)
    out = x + it * B
    return out, B, 1.01 * (it * Be + U * it * B + U * out), 1.01 * Be


def call_params(**over):
    return dict(R.BLOOM_DEFAULTS, **over)
