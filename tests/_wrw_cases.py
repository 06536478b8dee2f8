"""What tests/test_wrw_hostsim.py and tests/test_gpu_wrw.py share beyond the small SHAPES: inputs from {-1, 0, 1}, whose
weight gradient every correct summation order gives exactly, and impulse inputs that name the element of x a kernel
really multiplied.  Plain torch on whatever device it is handed; test infrastructure only."""
import torch

# the pixels of an impulse at 17 x 67 (tiles of 8 x 32: rows 8, 8, 1 and widths 32, 32, 3): the image's corners, both
# sides of the seam between four tiles, the 3-wide tile and the 1-row tile
IMPULSE_PIXELS = [(0, 0), (7, 31), (8, 32), (16, 66), (16, 64)]
# (B, Cin, Cout, H, W)
IMPULSE_SHAPES = [(2, 16, 16, 17, 67), (2, 96, 32, 17, 67)]


def impulse_rows(cout):
    return [0, 5, 15] + ([16, 31] if cout == 32 else [])


def ternary_case(shape, device="cpu"):
    """x, dy from {-1, 0, 1} and the fp64 weight gradient.  Every product is -1, 0 or 1 and every partial sum an integer
    of at most B H W in magnitude, so with B H W < 2^24 the fp32 accumulators, the reduction through LDS and the fp64
    sum over the workgroups are all exact: a correct kernel returns dw64 to the bit, in whatever order it adds."""
    B, Cin, Cout, H, W = shape
    assert B * H * W < 2 ** 24
    g = torch.Generator(device=device).manual_seed(7000 + 100 * Cin + Cout)
    x = torch.randint(-1, 2, (B, Cin, H + 2, W + 2), device=device, generator=g).float()
    dy = torch.randint(-1, 2, (B, Cout, H, W), device=device, generator=g).float()
    w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, device=device)
    dw64 = torch.ops.aten.convolution_backward(dy.double(), x.double(), w, None, [1, 1], [0, 0], [1, 1], False, [0, 0],
                                               1, [False, True, False])[1]
    return x, dy, dw64


def impulse_x(shape, device="cpu"):
    """x[n][ci][h][w] = 1 + its own flat index: a distinct integer below 2^24 for every element"""
    B, Cin, _, H, W = shape
    n = B * Cin * (H + 2) * (W + 2)
    assert n < 2 ** 24
    return (torch.arange(n, dtype=torch.float32, device=device) + 1).reshape(B, Cin, H + 2, W + 2)


def impulse_dy(shape, n, co, h, w, device="cpu"):
    B, _, Cout, H, W = shape
    dy = torch.zeros(B, Cout, H, W, device=device)
    dy[n, co, h, w] = 1.0
    return dy


def _decode(code, shape):
    B, Cin, _, H, W = shape
    c = float(code)
    if c != c or c != int(c) or not 1 <= c <= B * Cin * (H + 2) * (W + 2):
        return "no element of x"
    i = int(c) - 1
    i, w = divmod(i, W + 2)
    i, h = divmod(i, H + 2)
    n, ci = divmod(i, Cin)
    return f"x[n={n}][ci={ci}][h={h}][w={w}]"


def impulse_failure(got, x, shape, n, co, h, w):
    """None if dW (CPU, [Cout, Cin, 3, 3]) is what the impulse dy[n][co][h][w] = 1 must give, dW[co][ci][r][s] =
    x[n][ci][h + r][w + s] and zero in every other row; otherwise a sentence that names the first wrong entry, the code
    found there and the element of x that the code belongs to."""
    want = torch.zeros_like(got)
    want[co] = x[n, :, h:h + 3, w:w + 3]
    bad = ~(got == want)  # (a NaN is wrong, too)
    if not bool(bad.any()):
        return None
    o, ci, r, s = (int(v) for v in bad.nonzero()[0])
    found, expected = float(got[o, ci, r, s]), float(want[o, ci, r, s])
    what = "0" if found == 0 else f"{found!r}, which is {_decode(found, shape)}"
    exp = "0 (another row than the impulse's)" if o != co else f"{expected!r}, {_decode(expected, shape)}"
    return (f"impulse at dy[n={n}][co={co}][h={h}][w={w}] of {shape}: {int(bad.sum())} wrong entries, the first "
            f"dW[co={o}][ci={ci}][r={r}][s={s}] = {what}; expected {exp}")
