"""Two plain-numpy references of the depth decoder's glue (include/scsfm_nets.h; R: reflection pad by 1, E: ELU with
alpha 1, U: 2x nearest upsampling), and the shapes and input fills its tests share.

(a) `*_64`: the float64 yardstick.  np.pad(mode="reflect"), np.expm1, repeat, concatenate; the backward is their
    transpose, every sum in float64.  The ELU gradient is taken in the contract's result form: (r + 1) where r <= 0,
    else 1, with r the forward's fp32 result read as float64 (the kernels never see the ELU's input again).
(b) `*_32`: the order the header of csrc_nets/scsfm_decoder.hip promises, each step one float32 operation.  An entry
    (y, x) of an H x W plane is 0 + g[y+1][x+1], then + g[y+1][0] if x == 1, then + g[y+1][W+1] if x == W-2; the same
    three steps follow for padded row 0 if y == 1, then for padded row H+1 if y == H-2.  The four children of an
    upsampled element are added from 0 in row-major order; the ELU gradient is f * (r + 1) where r <= 0, else f.
"""
import numpy as np

U = 2.0 ** -24  # unit roundoff of fp32

# (B, C, H, W) of pad / elu_pad and (B, Ca, Cs, H, W) of up_cat_pad: the odd shapes, then the shapes around the kernels'
# 256-element chunk (a row of exactly 256 and 257 elements, the reflected column W-2 as the first lane of a chunk)
ODD_PAD = [(1, 3, 2, 2), (2, 5, 3, 3), (1, 4, 7, 5), (3, 2, 5, 263)]
ODD_UP = [(1, 3, 2, 1, 1), (1, 5, 0, 2, 3), (2, 7, 3, 3, 5), (1, 4, 4, 5, 131)]
CHUNK_PAD = [(1, 1, 2, 2), (1, 2, 3, 3)] + [(1, 1, 2, W) for W in (254, 255, 256, 257, 258)] + \
    [(2, 3, 3, 258), (3, 2, 5, 513)]
CHUNK_UP = [s for W in (127, 128, 129, 255, 256, 257) for s in ((1, 1, 1, 1, W), (1, 2, 0, 2, W))] + [(2, 3, 2, 5, 131)]
# DispResNet(50) on a 2 x 3 x 64 x 128 image: the pad input f4 and up_cat_pad at levels 4..0, with skips of 1024, 512
# and 256 channels
R50_PAD = [(2, 2048, 2, 4)]
R50_UP = [(2, 256, 1024, 2, 4), (2, 128, 512, 4, 8), (2, 64, 256, 8, 16), (2, 32, 64, 16, 32), (2, 16, 0, 32, 64)]

FLT_MIN, DENORM = np.float32(2.0 ** -126), np.float32(2.0 ** -149)
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, DENORM, -DENORM, FLT_MIN, -FLT_MIN, -1e-8, -17.5, -88.0,
                     -104.0, 3.4e38, -3.4e38, 1.0, -1.0], np.float32)


def fill(shape, kind, rng):
    """standard normal fp32 values; kind "special": about 40 % of them replaced by draws from SPECIALS"""
    v = rng.standard_normal(shape).astype(np.float32)
    if kind == "special":
        m = rng.random(shape) < 0.4
        v[m] = rng.choice(SPECIALS, size=int(m.sum()))
    return v


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def ulp_distance(a, b):
    """distance of two fp32 arrays in units in the last place (of their int32 patterns, -0 next to +0)"""
    def key(v):
        i = bits(v).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ---------------------------------------------------------------------------------------------- (a) float64

def _elu64(x):
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        return np.where(x > 0, x, np.expm1(x))


def _pad64(x):
    return np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="reflect")


def _up(x):
    return x.repeat(2, axis=2).repeat(2, axis=3)


def pad_fwd_64(x, elu):
    x = np.asarray(x, np.float64)
    return _pad64(_elu64(x) if elu else x)


def up_cat_pad_fwd_64(a, skip):
    x = _up(_elu64(a))
    if skip is not None and skip.shape[1]:
        x = np.concatenate([x, np.asarray(skip, np.float64)], 1)
    return _pad64(x)


def fold_64(gp):
    """the transpose of the reflection pad: rows 0 / H+1 onto rows 1 / H-2, then columns 0 / W+1 onto 1 / W-2"""
    gp = np.asarray(gp, np.float64)
    H, W = gp.shape[2] - 2, gp.shape[3] - 2
    with np.errstate(all="ignore"):
        t = gp[:, :, 1:-1, :].copy()
        t[:, :, 1, :] += gp[:, :, 0, :]
        t[:, :, H - 2, :] += gp[:, :, H + 1, :]
        g = t[:, :, :, 1:-1].copy()
        g[:, :, :, 1] += t[:, :, :, 0]
        g[:, :, :, W - 2] += t[:, :, :, W + 1]
    return g


def _children_64(g):
    with np.errstate(all="ignore"):
        return g[:, :, 0::2, 0::2] + g[:, :, 0::2, 1::2] + g[:, :, 1::2, 0::2] + g[:, :, 1::2, 1::2]


def _elu_slope_64(r):
    r = np.asarray(r, np.float64)
    return np.where(r <= 0, r + 1.0, 1.0)


def pad_bwd_64(gp, out, elu):
    """-> g_x, and the sum of |terms| * |E'| behind each entry (what a rounding bound scales with)"""
    slope = _elu_slope_64(out[:, :, 1:-1, 1:-1]) if elu else 1.0
    with np.errstate(all="ignore"):
        return fold_64(gp) * slope, fold_64(np.abs(np.asarray(gp, np.float64))) * np.abs(slope)


def up_cat_pad_bwd_64(gp, out, Ca):
    """-> g_a, g_skip (None without skip channels), and their sums of |terms| (* |E'| for g_a)"""
    g, mag = fold_64(gp), fold_64(np.abs(np.asarray(gp, np.float64)))
    slope = _elu_slope_64(out[:, :Ca, 1:-1:2, 1:-1:2])
    with np.errstate(all="ignore"):
        g_a, mag_a = _children_64(g[:, :Ca]) * slope, _children_64(mag[:, :Ca]) * np.abs(slope)
    if g.shape[1] == Ca:
        return g_a, None, mag_a, None
    return g_a, g[:, Ca:].copy(), mag_a, mag[:, Ca:].copy()


# ------------------------------------------------------------------------- (b) float32, in the documented order

def fold_32(gp):
    gp = np.ascontiguousarray(gp, np.float32)
    H, W = gp.shape[2] - 2, gp.shape[3] - 2
    acc = np.zeros(gp.shape[:2] + (H, W), np.float32)  # (+0: an entry with one term is 0 + g)
    with np.errstate(all="ignore"):
        # (to_row, from_padded_row): the entry's own row first, then padded row 0 onto row 1, then H+1 onto H-2
        for y, p in [(slice(None), slice(1, H + 1)), (1, 0), (H - 2, H + 1)]:
            acc[:, :, y, :] += gp[:, :, p, 1:-1]
            acc[:, :, y, 1] += gp[:, :, p, 0]
            acc[:, :, y, W - 2] += gp[:, :, p, W + 1]
    return acc


def _elu_grad_32(f, r):
    one = np.float32(1)
    with np.errstate(all="ignore"):
        return np.where(r <= 0, f * (r + one), f).astype(np.float32)


def pad_bwd_32(gp, out, elu):
    f = fold_32(gp)
    return _elu_grad_32(f, np.ascontiguousarray(out, np.float32)[:, :, 1:-1, 1:-1]) if elu else f


def up_cat_pad_bwd_32(gp, out, Ca):
    f = fold_32(gp)
    acc = np.zeros((f.shape[0], Ca, f.shape[2] // 2, f.shape[3] // 2), np.float32)
    with np.errstate(all="ignore"):
        for dy, dx in [(0, 0), (0, 1), (1, 0), (1, 1)]:
            acc += f[:, :Ca, dy::2, dx::2]
    g_a = _elu_grad_32(acc, np.ascontiguousarray(out, np.float32)[:, :Ca, 1:-1:2, 1:-1:2])
    return g_a, (f[:, Ca:].copy() if f.shape[1] > Ca else None)
