"""The cases tests/test_confidence_hostsim.py (host simulator) and tests/test_gpu_confidence.py (device) both run, each
against tests/confidence_oracle.py bit for bit.

A backend gives `pairs(c2w, K, radius)`, `weights(depth, pair, **kw)` on numpy arrays, `volume(dims, origin, voxel, trunc,
max_weight, frames_per_launch)` -- an object with scsfm_hip.fusion.Volume's integrate (with ``weight=``) and a `planes`
array -- and `dev` / `host` to move arrays.  The world is generated: a static height field z = h(x, y) seen by cameras
that move sideways and turn a little, its depth found per pixel by a fixed-point iteration along the ray (float64), at
12 x 20 (W a multiple of 4: the 16-byte path) and 37 x 61 (not; 2257 pixels are three workgroups, the last one partial).
The references are computed once (cached) and read-only.  Test infrastructure only."""
from __future__ import annotations

import functools

import numpy as np

import confidence_oracle as CO
import _fusion_cases as FC
from _fusion_cases import pose, same_bits

f32 = np.float32
HW = (12, 20)
HW_ODD = (37, 61)
K = FC.K                                                                        # f = 12, centre (9.5, 5.5)
K_ODD = np.array([[37.0, 0, 29.5], [0, 37.0, 17.5], [0, 0, 1]], np.float32)
K_POW2 = np.array([[16.0, 0, 9.5], [0, 16.0, 5.5], [0, 0, 1]], np.float32)      # shifts of whole pixels are exact
MAX_DEPTH = 4.0


def height(x, y):
    return 2.0 + 0.15 * np.sin(1.7 * x + 0.3) * np.cos(1.3 * y) + 0.1 * x


def render(c2w, Kc, hw, iters=40):
    """the depth [H, W] float64 of the height field from the camera: s with c + s R (x_n, y_n, 1) on the surface"""
    H, W = hw
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    ray = np.stack([(px - Kc[0, 2]) / Kc[0, 0], (py - Kc[1, 2]) / Kc[1, 1], np.ones((H, W))], -1) @ c2w[:, :3].T
    s = np.full((H, W), 2.0)
    for _ in range(iters):
        p = c2w[:, 3] + s[..., None] * ray
        s = (height(p[..., 0], p[..., 1]) - c2w[2, 3]) / ray[..., 2]
    return s


def path(n, skew=0.0):
    """n camera-to-world poses moving along x, turning a little"""
    return np.stack([pose(0.02 * k - 0.04, 0.01 * k, (0.08 * k - 0.2, 0.02 * k, 0.03 * k), skew=skew * (k % 3))
                     for k in range(n)])


@functools.lru_cache(maxsize=None)
def world(n, odd):
    """-> (depth [n, H, W] float32, c2w [n, 3, 4] float64, K), read-only"""
    Kc, hw = (K_ODD, HW_ODD) if odd else (K, HW)
    c2w = path(n)
    noise = np.random.default_rng(7 + n + 100 * odd).standard_normal((n,) + hw)     # 1 % of the depth: the weights spread
    depth = (np.stack([render(p, Kc, hw) for p in c2w]) * (1 + 0.01 * noise)).astype(np.float32)
    for a in (depth, c2w):
        a.setflags(write=False)
    return depth, c2w, Kc


def _as_disp(depth):
    with np.errstate(all="ignore"):
        return (f32(1) / depth).astype(np.float32)


@functools.lru_cache(maxsize=1)
def cases():
    out = {}

    def add(name, depth, c2w, Kc, radius=1, is_disp=False, edit=None, **kw):
        depth = np.array(depth, np.float32)
        if edit is not None:
            edit(depth)
        if is_disp:
            depth = _as_disp(depth)
        depth.setflags(write=False)
        out[name] = dict(depth=depth, c2w=np.asarray(c2w, np.float64), K=Kc, radius=radius,
                         kw=dict(is_disp=is_disp, max_depth=MAX_DEPTH, **kw))

    for odd in (False, True):
        tag = "odd" if odd else "w4"
        for is_disp in (False, True):
            kind = "disp" if is_disp else "depth"
            for n, radius in ((5, 1), (5, 2), (2, 4), (1, 1)):
                add(f"n{n}_r{radius}_{tag}_{kind}", *world(n, odd), radius=radius, is_disp=is_disp)
    add("min_views_2", *world(5, False), radius=1, min_views=2)
    add("floor", *world(5, True), radius=2, floor=0.99)
    add("max", *world(5, True), radius=2, reduce="max")
    add("max_floor_disp", *world(5, False), radius=2, reduce="max", floor=0.99, is_disp=True, min_views=2)

    # identity rotations, constant depth 2, f = 16: a step of 0.125 along x (y) moves the picture by one pixel exactly
    flat = np.full((3,) + HW, 2.0, np.float32)
    step_x = np.stack([pose(pos=(0.125 * k, 0.0, 0.0)) for k in range(3)])
    step_y = np.stack([pose(pos=(0.0, 0.125 * k, 0.0)) for k in range(3)])
    add("integer_x", flat, step_x, K_POW2)
    add("integer_y", flat, step_y, K_POW2)
    # 0.3 of a pixel: u = px - 0.3 towards the next frame, so column 0 must lose that neighbour (not be truncated to 0)
    frac = np.stack([pose(pos=(0.3 * 0.125 * k, 0.0, 0.0)) for k in range(3)])
    add("fraction_x", flat, frac, K_POW2)

    def own(depth):
        depth[1, 2, 3], depth[1, 2, 4], depth[1, 2, 5], depth[1, 2, 6] = 0.0, np.nan, 7.5, -1.0
    add("own_depth", flat, frac, K_POW2, edit=own)

    def own_disp(depth):   # (edited as depths; 1 / inf is the disparity 0, 1 / 1e-30 overflows)
        depth[1, 2, 3], depth[1, 2, 4], depth[1, 2, 5] = np.inf, np.nan, 1e-30
    add("own_disp", flat, frac, K_POW2, is_disp=True, edit=own_disp)

    def taps(depth):
        depth[2, 5, 7], depth[0, 8, 12] = 0.0, np.nan
    add("taps", flat, frac, K_POW2, edit=taps)
    add("taps_disp", flat, frac, K_POW2, is_disp=True, edit=taps)
    # the middle frame looks the other way: every point of its neighbours lies behind it, and its points behind them
    away = frac.copy()
    away[1] = pose(np.pi, 0.0, (0.0375, 0.0, 0.0))
    add("behind", flat, away, K_POW2)
    # the same frame three times at one pose, turned and not
    # (the smooth surface: where u comes back an ulp off px, a depth that changes little between two pixels still gives
    # m = fl(1 - 1e-8) = 1; with the noisy depth of world() such a pixel may end at 1 - 2^-24)
    turned = path(3)[1]
    add("identical", np.stack([render(turned, K_ODD, HW_ODD)] * 3), np.stack([turned] * 3), K_ODD)
    add("identical_pow2", np.stack([world(3, False)[0][0]] * 3), np.stack([pose()] * 3), K_POW2)
    return out


NAMES = tuple(f"n{n}_r{r}_{tag}_{kind}" for tag in ("w4", "odd") for kind in ("depth", "disp")
              for n, r in ((5, 1), (5, 2), (2, 4), (1, 1))) + (
    "min_views_2", "floor", "max", "max_floor_disp", "integer_x", "integer_y", "fraction_x", "own_depth", "own_disp", "taps",
    "taps_disp", "behind", "identical", "identical_pow2")


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (pair, weight, count) of the oracle (computed once; read-only)"""
    case = cases()[name]
    pair = CO.pairs(case["c2w"], case["K"], case["radius"])
    weight, count = CO.weights(case["depth"], pair, detail=True, **case["kw"])
    for a in (pair, weight, count):
        a.setflags(write=False)
    return pair, weight, count


def check(name, backend):
    case = cases()[name]
    pair, weight, _ = reference(name)
    got_pair = backend.pairs(case["c2w"], case["K"], case["radius"])
    assert same_bits(got_pair, pair), f"{name}: the pair records differ"
    got = backend.weights(case["depth"], got_pair, **case["kw"])
    assert got.dtype == np.float32 and same_bits(got, weight), f"{name}: the weights differ"
    return weight


# ---- pairs ----

def pair_poses():
    """rigid poses, then poses whose 3 x 3 is off orthonormal (the general inverse)"""
    return dict(rigid=path(5), skewed=path(5, skew=0.02))


# ---- integration ----

VOLUMES = dict(scalar=dict(dims=(37, 19, 22), origin=(-1.85, -0.9, 0.45), voxel=0.1),
               vector=dict(dims=(40, 16, 12), origin=(-2.0, -0.8, 1.45), voxel=0.1))


@functools.lru_cache(maxsize=1)
def fuse_cases():
    rng = np.random.default_rng(31)
    out = {}

    def add(name, volume, poses, images, weight, max_weight=64.0):
        call = FC._call(poses, rng, images=images)
        F = len(call["depth"])
        w = weight(F)
        w.setflags(write=False)
        out[name] = dict(name=name, **VOLUMES[volume], max_weight=max_weight, call=call, weight=w)

    ones = lambda F: np.ones((F,) + HW, np.float32)
    some = lambda F: rng.uniform(0.05, 1.0, (F,) + HW).astype(np.float32)

    def skips(F):
        w = some(F)
        w[0, 2:5, 3:9], w[1, :, :4], w[2, 6:9, 10:16], w[3, 1:3, :] = 0.0, -1.0, np.nan, 1.5
        w[4, 4, 4], w[4, 5, 5] = 1.0, np.nextafter(f32(1), f32(2))
        return w
    for volume in ("scalar", "vector"):
        for images in (True, False):
            tag = f"{volume}_{'image' if images else 'plain'}"
            add(f"ones_{tag}", volume, FC._straddle(5, rng), images, ones)
            add(f"fractional_{tag}", volume, FC._straddle(5, rng), images, some)
    add("skips_scalar_image", "scalar", FC._straddle(5, rng), True, skips)
    add("skips_vector_plain", "vector", FC._straddle(5, rng), False, skips)
    add("max_weight_scalar_image", "scalar", FC._straddle(8, rng)[4:6] * 4, True, some, max_weight=2.5)
    add("max_weight_vector_plain", "vector", FC._straddle(8, rng)[4:6] * 4, False, some, max_weight=2.5)
    return out


FUSE_NAMES = tuple(f"{k}_{v}_{i}" for v in ("scalar", "vector") for i in ("image", "plain") for k in ("ones", "fractional")) + (
    "skips_scalar_image", "skips_vector_plain", "max_weight_scalar_image", "max_weight_vector_plain")


@functools.lru_cache(maxsize=None)
def fuse_reference(name):
    case = fuse_cases()[name]
    vol = CO.Volume(case["dims"], case["origin"], case["voxel"], None, case["max_weight"])
    vol.integrate(**case["call"], weight=case["weight"])
    vol.planes.setflags(write=False)
    return vol


def run_fuse(case, backend, frames_per_launch, weighted=True, one_call=True):
    vol = backend.volume(case["dims"], case["origin"], case["voxel"], None, case["max_weight"], frames_per_launch)
    call = case["call"]
    F = len(call["depth"])
    for f0, f1 in ((0, F),) if one_call else tuple((f, f + 1) for f in range(F)):
        vol.integrate(backend.dev(call["depth"][f0:f1]),
                      None if call["images"] is None else backend.dev(call["images"][f0:f1]),
                      backend.dev(call["c2w"][f0:f1]), backend.dev(call["K"]), is_disp=call["is_disp"], near=call["near"],
                      max_depth=call["max_depth"], **(dict(weight=backend.dev(case["weight"][f0:f1])) if weighted else {}))
    return backend.host(vol.planes)


PLANES = ("tsdf", "weight", "r", "g", "b")


def check_fuse(name, backend):
    """against the oracle bit for bit at 5 (8), 2 and 1 frames per launch and as F calls of one frame; a weight of all
    ones also against the unweighted library"""
    case = fuse_cases()[name]
    ref = fuse_reference(name)
    F = len(case["call"]["depth"])
    for fpl, one_call in ((F, True), (2, True), (1, True), (F, False)):
        planes = run_fuse(case, backend, fpl, one_call=one_call)
        for k, plane in enumerate(PLANES):
            assert same_bits(planes[k], ref.planes[k]), f"{name}: the {plane} plane differs ({fpl} a launch, {one_call})"
    if name.startswith("ones"):
        plain = run_fuse(case, backend, F, weighted=False)
        for k, plane in enumerate(PLANES):
            assert same_bits(plain[k], ref.planes[k]), f"{name}: the {plane} plane differs from the unweighted library's"
    return ref


# ---- does it do its job: an object that moves against the poses ----

MOVING = dict(n=6, zo=1.75, half=4, dims=(50, 32, 30), origin=(-1.2, -0.8, 1.15), voxel=0.05, min_weight=2.0)


@functools.lru_cache(maxsize=1)
def moving_world():
    """six 37 x 61 frames of the height field; in frame k a plate of 8 x 8 pixels, parallel to the picture plane, stands
    where an object that comes towards the cameras (0.1 a frame, from the world depth zo) is seen -> dict(depth, c2w, K, patch [n, H, W] bool, box)"""
    n, zo, half = MOVING["n"], MOVING["zo"], MOVING["half"]
    depth, c2w, Kc = world(n, True)
    depth = depth.copy()
    H, W = HW_ODD
    patch = np.zeros((n, H, W), bool)
    centres = []
    for k in range(n):
        centre = np.array([0.2 - 0.03 * k, 0.01 * k - 0.05, zo - 0.1 * k])
        centres.append(centre)
        q = c2w[k][:, :3].T @ (centre - c2w[k][:, 3])
        uc, vc = Kc[0, 0] * q[0] / q[2] + Kc[0, 2], Kc[1, 1] * q[1] / q[2] + Kc[1, 2]
        x0, y0 = int(round(uc)) - half, int(round(vc)) - half
        assert 1 <= x0 and x0 + 2 * half < W - 1 and 1 <= y0 and y0 + 2 * half < H - 1, (k, x0, y0)
        patch[k, y0:y0 + 2 * half, x0:x0 + 2 * half] = True
        px, py = np.meshgrid(np.arange(W), np.arange(H))
        ray = np.stack([(px - Kc[0, 2]) / Kc[0, 0], (py - Kc[1, 2]) / Kc[1, 1], np.ones((H, W))], -1) @ c2w[k][:, :3].T
        plate = ((centre[2] - c2w[k][2, 3]) / ray[..., 2]).astype(np.float32)
        depth[k] = np.where(patch[k], plate, depth[k])
    centres = np.array(centres)
    grow = np.array([0.3, 0.3, 0.1])
    box = (centres.min(0) - grow, centres.max(0) + grow)
    for a in (depth, patch):
        a.setflags(write=False)
    return dict(depth=depth, c2w=c2w, K=Kc, patch=patch, box=box)


def moving_medians(weight, count):
    """-> (the median weight on the patches, the median weight on the static pixels that have a neighbour)"""
    patch = moving_world()["patch"]
    return float(np.median(weight[patch])), float(np.median(weight[~patch & (count > 0)]))


def moving_counts(xyz):
    """-> (surface points inside the object's swept box, outside it)"""
    lo, hi = moving_world()["box"]
    inside = ((xyz >= lo) & (xyz <= hi)).all(axis=1)
    return int(inside.sum()), int((~inside).sum())


@functools.lru_cache(maxsize=1)
def moving_reference():
    """the oracle alone -> dict(weight, count, medians, floor, plain (inside, outside), weighted (inside, outside))"""
    w = moving_world()
    pair = CO.pairs(w["c2w"], w["K"], 1)
    weight, count = CO.weights(w["depth"], pair, is_disp=False, max_depth=MAX_DEPTH, detail=True)
    on, off = moving_medians(weight, count)
    floor = float(f32(0.5 * (on + off)))
    cut = CO.weights(w["depth"], pair, is_disp=False, max_depth=MAX_DEPTH, floor=floor)
    counts = []
    for wt in (None, cut):
        vol = CO.Volume(MOVING["dims"], MOVING["origin"], MOVING["voxel"])
        vol.integrate(w["depth"], None, w["c2w"], w["K"], is_disp=False, near=0.05, max_depth=MAX_DEPTH, weight=wt)
        counts.append(moving_counts(vol.extract(MOVING["min_weight"])[0]))
    return dict(weight=weight, count=count, medians=(on, off), floor=floor, cut=cut, plain=counts[0], weighted=counts[1])
