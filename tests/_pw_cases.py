"""What tests/test_pw_hostsim.py and tests/test_gpu_pw.py share: the shapes, ATen's references and the bound.

Shapes are (B, Cin, Cout, H, W, stride) with H x W the INPUT's size; the output has Ho = (H - 1) // s + 1 rows.

Bound per entry:  |got - ref64| <= 2 max|ref32 - ref64| + 8 u S,  with ref64 ATen's result in fp64, ref32 ATen's fp32
result of the same op, S the op on the operands' absolute values in fp64 and u = 2^-24 (tests/test_gpu_wrw.py's).  For
the data gradient the positions the stride skips are checked for exact zeros besides (`unsampled`)."""
import torch

U = 2.0 ** -24
SHAPES = [
    (2, 64, 128, 6, 10, 2),    # the plain case
    (1, 64, 128, 7, 11, 2),    # odd H and W: the last row and column are sampled
    (3, 128, 256, 5, 35, 2),   # an output row of 18 pixels: more than one 16-pixel block, ragged
    (2, 256, 512, 2, 4, 2),    # fewer pixels than one K step
    (1, 64, 128, 1, 1, 2),     # a single pixel
    (5, 64, 128, 9, 67, 2),    # several partials
    (2, 512, 256, 3, 7, 1),    # stride 1, weight gradient only
]
# more 32-pixel chunks (7 x 5, the fifth ragged) than the 512 / 16 = 32 workgroups a (Cout, Cin) tile gets: some
# workgroups walk two chunks, which is what the prefetch under the multiplication and the second commit are for
MULTI = [(7, 256, 512, 11, 50, 2)]
DGRAD_SHAPES = [s for s in SHAPES + MULTI if s[5] == 2]
ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]  # noqa: E731


def out_size(n, stride):
    return (n - 1) // stride + 1


def aten_wgrad(x, dy, stride):
    w = torch.zeros(dy.shape[1], x.shape[1], 1, 1, dtype=x.dtype, device=x.device)
    return torch.ops.aten.convolution_backward(dy, x, w, None, [stride] * 2, [0, 0], [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1]


def aten_dgrad(dy, w, H, W, stride=2):
    x = torch.zeros(dy.shape[0], w.shape[1], H, W, dtype=dy.dtype, device=dy.device)
    return torch.ops.aten.convolution_backward(dy, x, w, None, [stride] * 2, [0, 0], [1, 1], False, [0, 0], 1,
                                               [True, False, False])[0]


def operands(shape, device="cpu", ternary=False):
    """x, dy, w (fp32) of a shape; ternary: from {-1, 0, 1}, for which every summation order is exact"""
    B, Cin, Cout, H, W, s = shape
    g = torch.Generator().manual_seed(1000 * Cin + 10 * H + W + s)
    sizes = (B, Cin, H, W), (B, Cout, out_size(H, s), out_size(W, s)), (Cout, Cin, 1, 1)
    if ternary:
        return tuple((torch.randint(-1, 2, n, generator=g).float()).to(device) for n in sizes)
    x, dy, w = (torch.randn(n, generator=g) for n in sizes)
    return x.to(device), dy.to(device), (w / Cin ** 0.5).to(device)


def wgrad_refs(x, dy, stride):
    """-> ref64, max|ref32 - ref64|, S of the weight gradient"""
    ref64 = aten_wgrad(x.double(), dy.double(), stride)
    yard = float((aten_wgrad(x, dy, stride).double() - ref64).abs().max())
    return ref64, yard, aten_wgrad(x.double().abs(), dy.double().abs(), stride)


def dgrad_refs(dy, w, H, W):
    """-> ref64, max|ref32 - ref64|, S of the stride-2 data gradient"""
    ref64 = aten_dgrad(dy.double(), w.double(), H, W)
    yard = float((aten_dgrad(dy, w, H, W).double() - ref64).abs().max())
    return ref64, yard, aten_dgrad(dy.double().abs(), w.double().abs(), H, W)


def unsampled(dx):
    """the entries of dx[B, Cin, H, W] at positions a stride-2 convolution does not read, as one flat tensor"""
    return torch.cat([dx[:, :, 1::2, :].reshape(-1), dx[:, :, 0::2, 1::2].reshape(-1)])


def worst(got, ref64, yard, S):
    """the largest |got - ref64| / bound over the entries (an exact zero where the bound is zero counts as 0); NaN or inf
    anywhere in `got` gives inf"""
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err, bound = (got.double() - ref64).abs(), 2 * yard + 8 * U * S
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)  # (x / 0 = inf for x > 0)
    return float(ratio.max())
