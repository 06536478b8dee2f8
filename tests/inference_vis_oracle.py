"""What run_inference.py computes around the network, written out in numpy: the input normalisation, the two colour
tables and the two pictures.  Independent of scsfm_hip.visualise (which the tests judge with it) and of matplotlib
(against which tests/test_inference_vis_reference.py judges it).

    picture = uint8(float32(255) * float32(cmap(map / max_value)))          (H, W, 4)

with matplotlib's Colormap.__call__ on a float32 array: xa = norm * N in float32, xa == N -> N - 1, xa < 0 -> the
under colour (entry 0), xa >= N -> the over colour (entry N - 1), NaN -> the bad colour (0, 0, 0, 0), otherwise the
entry at xa truncated toward zero.
"""
import numpy as np

BONE_N, RAINBOW_N = 10000, 1000
BONE_STOPS = {
    "red": ((0., 0.), (0.746032, 0.652778), (1.0, 1.0)),
    "green": ((0., 0.), (0.365079, 0.319444), (0.746032, 0.777778), (1.0, 1.0)),
    "blue": ((0., 0.), (0.365079, 0.444444), (1.0, 1.0)),
}
RAINBOW_STOPS = ((0.000, (1.00, 0.00, 0.00)), (0.400, (1.00, 1.00, 0.00)), (0.600, (0.00, 1.00, 0.00)),
                 (0.800, (0.00, 0.00, 1.00)), (1.000, (0.60, 0.00, 1.00)))


def _ramp(n, xs, ys):
    """One channel: piecewise linear through (xs, ys) at linspace(0, 1, n), in float64, written as a loop."""
    out = np.empty(n, dtype=np.float64)
    grid = np.linspace(0.0, 1.0, n)
    out[0], out[-1] = ys[0], ys[-1]
    for k in range(1, n - 1):
        i = int(np.searchsorted(np.asarray(xs, dtype=np.float64), grid[k]))
        dist = (grid[k] - xs[i - 1]) / (xs[i] - xs[i - 1])
        out[k] = dist * (ys[i] - ys[i - 1]) + ys[i - 1]
    return np.clip(out, 0.0, 1.0)


def to_bytes(rgba):
    return (np.float32(255) * np.asarray(rgba).astype(np.float32)).astype(np.uint8)


_tables = {}


def table(name):
    """uint8 [N, 4] of 'bone' or 'rainbow'."""
    if name not in _tables:
        if name == "bone":
            chans = [_ramp(BONE_N, [s[0] for s in BONE_STOPS[c]], [s[1] for s in BONE_STOPS[c]])
                     for c in ("red", "green", "blue")]
            n = BONE_N
        elif name == "rainbow":
            xs = [s[0] for s in RAINBOW_STOPS]
            chans = [_ramp(RAINBOW_N, xs, [s[1][i] for s in RAINBOW_STOPS]) for i in range(3)]
            n = RAINBOW_N
        else:
            raise KeyError(name)
        _tables[name] = to_bytes(np.stack(chans + [np.ones(n)], axis=1))
    return _tables[name]


def normalise(frames):
    """uint8 [N, H, W, 3] -> float32 [N, 3, H, W]: (x / 255 - 0.45) / 0.225 in float32."""
    x = np.asarray(frames).astype(np.float32).transpose(0, 3, 1, 2)
    return ((x / np.float32(255) - np.float32(0.45)) / np.float32(0.225)).astype(np.float32)


def image_max(maps):
    """float32 [N, H, W] -> float32 [N]; NaN when the image holds one (numpy's max propagates it)."""
    maps = np.asarray(maps, dtype=np.float32)
    return maps.reshape(len(maps), -1).max(axis=1)


def picture(one, name, max_value=None, reciprocal=False):
    """One float32 [H, W] map -> uint8 [H, W, 4]."""
    if reciprocal and max_value is None:
        raise ValueError("a reciprocal picture needs a max_value")
    tab = table(name)
    n = len(tab)
    one = np.asarray(one, dtype=np.float32)
    with np.errstate(all="ignore"):
        if reciprocal:
            one = (np.float32(1) / one).astype(np.float32)
        d = one.max() if max_value is None else np.float32(max_value)
        xa = ((one / np.float32(d)).astype(np.float32) * np.float32(n)).astype(np.float32)
        idx = np.trunc(np.where(np.isfinite(xa), xa, 0)).astype(np.int64)
    idx = np.where(xa == n, n - 1, idx)
    idx = np.where(xa < 0, 0, idx)
    idx = np.where(xa >= n, n - 1, idx)
    out = tab[np.clip(idx, 0, n - 1)].copy()
    out[np.isnan(xa)] = 0
    return out


def colourise(maps, name, max_value=None, reciprocal=False):
    """float32 [N, H, W] -> uint8 [N, H, W, 4], every image on its own."""
    return np.stack([picture(m, name, max_value, reciprocal) for m in np.asarray(maps, dtype=np.float32)])


def disparity_and_depth(disp):
    """The two pictures run_inference.py writes for each disparity map of float32 [N, H, W]."""
    return colourise(disp, "bone"), colourise(disp, "rainbow", max_value=10, reciprocal=True)
