"""The maps on which the colour-mapped pictures are judged, for the host simulator and for the GPU alike: every shape at
which the kernels take another path (one pixel; fewer pixels than a lane group; an odd size over several blocks with
images that start off the 16-byte boundary; a multiple-of-nothing width), three images of different maxima so that a
global maximum or a wrong image stride shows, and one planted value per case."""
import numpy as np

SHAPES = [(1, 1, 1), (2, 3, 5), (3, 37, 53), (1, 64, 67)]
# (colormap, max_value, reciprocal): the disparity picture, the depth picture, and a fixed divisor without reciprocal
CALLS = [("bone", None, False), ("rainbow", 10, True), ("rainbow", 10, False)]
SCALES = (1.0, 2.5, 0.3)


def base(shape, seed=0):
    """Disparities in (0.01, 0.91) times a scale that differs from image to image."""
    rng = np.random.default_rng(seed)
    maps = (rng.random(shape, dtype=np.float32) * np.float32(0.9) + np.float32(0.01)).astype(np.float32)
    for n in range(shape[0]):
        maps[n] *= np.float32(SCALES[n % len(SCALES)])
    return maps


def _max_last(m):
    m[:, -1, -1] = m.reshape(len(m), -1).max(axis=1) * np.float32(1.5)


def _equals_max_value(m):
    m[:, 1, 2] = np.float32(10.0)  # CALLS[2]: xa == N exactly
    m[0, 2, 3] = np.float32(10.000001)


def _zero_disparity(m):
    m[1, 5, 7] = 0.0  # depth +inf
    m[2, 0, 0] = -0.0  # depth -inf


def _negative(m):
    m[0, 3, 4] = -0.25
    m[2, 36, 52] = -1e-30


def _nan_in_one_image(m):
    m[1, 17, 29] = np.nan


def _all_zero_image(m):
    m[2] = 0.0


def _mostly_far(m):
    m *= np.float32(0.12)  # image 0: disparities below 0.1 for most pixels, depth over 10


def _infinite(m):
    m[0, 4, 4] = np.inf  # the maximum itself: inf / inf is NaN there, 0 elsewhere


PLANTS = {"max_last": _max_last, "equals_max_value": _equals_max_value, "zero_disparity": _zero_disparity,
          "negative": _negative, "nan_in_one_image": _nan_in_one_image, "all_zero_image": _all_zero_image,
          "mostly_far": _mostly_far, "infinite": _infinite}


def planted(name):
    m = base((3, 37, 53), seed=1)
    PLANTS[name](m)
    return m


def all_bytes():
    """Two uint8 [2, 5, 7, 3] batches (210 bytes each) that hold every byte value between them: 0 .. 209 and
    46 .. 255."""
    n = 2 * 5 * 7 * 3
    return [np.arange(n).astype(np.uint8).reshape(2, 5, 7, 3), np.arange(256 - n, 256).astype(np.uint8).reshape(2, 5, 7, 3)]
