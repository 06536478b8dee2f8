"""The inputs shared by the depth-visualisation tests (oracle against reference, kernels on the simulator and on the
GPU): shapes, planted values, ragged sets and evaluation sets.  Everything is generated from seeds."""
import numpy as np

DTYPES = (np.float32, np.float64)
# n = 1, 2, 3, 15, 20 give the weights t = 0, .95, .9, .3, .05: both branches of the interpolation
SMALL_SHAPES = ((1, 1), (1, 2), (1, 3), (3, 5), (4, 5), (37, 53), (64, 130))
LARGE_SHAPE = (375, 1242)
# 41 elements: float32 forms the virtual index 40 * 0.95 = 38.0 (lo = 38, t = 0), float64 37.99999999999999 (lo = 37)
SPLIT_SHAPE = (1, 41)


def base(shape, dtype, seed=0):
    return np.random.default_rng(seed).uniform(0.5, 80.0, shape).astype(dtype)


def _constant(m):
    m[1] = 3.0


def _top6(m):
    flat = m[1].ravel()
    k = int(np.ceil(0.06 * flat.size)) + 1
    flat[np.argsort(flat)[:k]] = 0.5  # the smallest depths are the largest inverse depths: vmax sits on a plateau


def _nan(m):
    m[1, 3, 4] = np.nan


def _inf(m):
    m[1, 2, 2] = -1e-6  # x + 1e-6 == 0 in both precisions
    m[2, 0, :] = -1e-6  # more than 5 % of 37 x 53 is 99 pixels: a row of 53 stays below, so vmax stays finite here ...
    m[0].ravel()[:150] = -1e-6  # ... and is +inf here (inf - inf in the interpolation: NaN, as in numpy)


def _negative(m):
    m[1, 5, 5:9] = -5.0
    m[2, :4] *= -1


def _zeros(m):
    m[1, 0, 0] = 0.0
    m[2].ravel()[::9] = 0.0  # 11 % holes: vmax is 1e6


PLANTS = {"constant": _constant, "top6_equal": _top6, "nan_in_one_image": _nan, "inf": _inf, "negative": _negative,
          "zeros": _zeros}


def planted(name, dtype, shape=(3, 37, 53)):
    m = base(shape, dtype, seed=sorted(PLANTS).index(name) + 1)
    PLANTS[name](m)
    return m


def ragged(dtype, seed=7):
    """Maps of different sizes; (1, 3) makes the next packed offset a multiple of 4 only through padding."""
    sizes = ((3, 5), (1, 3), (37, 53), (1, 1), (4, 5), (1, 41))
    return [base(s, dtype, seed + i) for i, s in enumerate(sizes)]


def eval_set(dataset, gdt, pdt, seed=3, skip=True, small=False):
    """(gt_depths, pred_depths): four images; the third prediction has mean exactly -1 when ``skip``.  KITTI's GT is
    ragged and sparse (zeros), NYU's one array with a hole."""
    rng = np.random.default_rng(seed)
    h, w = (4, 9) if small else (8, 26)
    pred = rng.uniform(0.1, 3.0, (4, h, w)).astype(pdt)
    if skip:
        pred[2] = -1.0
    if dataset == "kitti":
        sizes = ((13, 41), (12, 40), (13, 41), (14, 39)) if small else ((37, 123), (36, 122), (37, 123), (38, 121))
        gts = []
        for s in sizes:
            g = rng.uniform(1.0, 90.0, s)
            g[rng.uniform(size=s) < 0.4] = 0.0
            gts.append(g.astype(gdt))
        return gts, pred
    gt = rng.uniform(0.5, 11.0, (4, 19, 25)).astype(gdt)
    gt[1, 3:5, 2:9] = 0.0
    return gt, pred


def photos(sizes, seed=11):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
