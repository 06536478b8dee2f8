"""Inputs, references and the bound for the tests of the tail-backward kernel (csrc_dgrad/scsfm_decoder_dgrad.hip):
shared by tests/test_dgrad_hostsim.py (CPU, host simulator) and tests/test_gpu_dgrad.py (GPU).

The ATen chain of the tail, from the ELU's input x (conv (0, 1)'s output with its bias added):

    out = alpha * sigmoid(conv2d(reflection_pad(elu(x)), w) + bias_h) + beta

ref32 / ref64 are its autograd gradients in fp32 / fp64; the kernel gets what the fp32 forward saved (the padded ELU
result q, the sigmoid y), the output gradient and w.  S is the same backward on absolute values: |elu'| times the fold of
conv_transpose(|g|, |w|).  Per entry  |new32 - ref64| <= 2 max|ref32 - ref64| + 8 u S,  u = 2^-24; the sums use the sums of
S over what they add.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
ALPHA, BETA = 10.0, 0.01
C = 16
# (B, H, W): every pixel a corner; odd sizes; one tile; three tiles down and two across with partial ones; three across
SHAPES = [(1, 2, 2), (2, 3, 5), (1, 5, 7), (2, 17, 67), (1, 9, 130)]


def chain(x, w, bias_h):
    q = F.pad(F.elu(x), (1, 1, 1, 1), mode="reflect")
    y = torch.sigmoid(F.conv2d(q, w, bias_h))
    return q, y, ALPHA * y + BETA


def fold(gq):
    """the reflection pad's backward: [B, C, H + 2, W + 2] -> [B, C, H, W]"""
    z = torch.zeros(gq.shape[0], gq.shape[1], gq.shape[2] - 2, gq.shape[3] - 2, dtype=gq.dtype, requires_grad=True)
    return torch.autograd.grad(F.pad(z, (1, 1, 1, 1), mode="reflect"), z, gq)[0]


def case(shape, seed=0):
    """-> dict of fp32 inputs of the kernel (numpy) and the references (fp64 numpy)"""
    B, H, W = shape
    gen = torch.Generator().manual_seed(1000 * H + W + seed)
    x = torch.randn(B, C, H, W, generator=gen)
    w = torch.randn(1, C, 3, 3, generator=gen) / 12
    bias_h = torch.randn(1, generator=gen)
    g_out = torch.randn(B, 1, H, W, generator=gen)
    res = {}
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        xs, ws, bs = (t.to(dt).requires_grad_(True) for t in (x, w, bias_h))
        q, y, out = chain(xs, ws, bs)
        g_x, g_bh = torch.autograd.grad(out, (xs, bs), g_out.to(dt))
        res[name] = dict(q=q.detach(), y=y.detach(), g_b=g_x, g_bias_b=g_x.sum((0, 2, 3)), g_bias_head=g_bh)
    y64 = res["64"]["y"]
    g64 = g_out.double() * ALPHA * y64 * (1 - y64)
    x64 = x.double()
    d_elu = torch.where(x64 > 0, torch.ones_like(x64), torch.exp(x64))
    S = d_elu * fold(F.conv_transpose2d(g64.abs(), w.double().abs()))
    n = lambda t: t.detach().numpy()  # noqa: E731
    return dict(q=n(res["32"]["q"]), y=n(res["32"]["y"]), g_out=n(g_out), w=n(w),
                ref32={k: n(v) for k, v in res["32"].items()}, ref64={k: n(v) for k, v in res["64"].items()},
                g64=n(g64), S=dict(g_b=n(S), g_bias_b=n(S.sum((0, 2, 3))), g_bias_head=n(g64.abs().sum().reshape(1))))


def ratio(new32, ref32, ref64, S):
    """the worst entry's |new32 - ref64| over its bound"""
    yard = float(np.abs(ref32.astype(np.float64) - ref64).max())
    return float((np.abs(new32.astype(np.float64) - ref64) / (2 * yard + 8 * U * S + 1e-300)).max())


def exact_case(shape, seed=0):
    """null-y mode on values whose every product and sum is exact in fp32: g in {-1, 0, 1}, w in {-1, 0, 0.5, 1},
    E in {-0.5, 0, 1, 2} -> q, g, w (fp32 numpy)"""
    B, H, W = shape
    rng = np.random.default_rng(7 * H + W + seed)
    g = rng.choice(np.array([-1, 0, 1], np.float32), (B, 1, H, W))
    w = rng.choice(np.array([-1, 0, 0.5, 1], np.float32), (1, C, 3, 3))
    e = rng.choice(np.array([-0.5, 0, 1, 2], np.float32), (B, C, H, W))
    return np.pad(e, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="reflect"), g, w


def tail_ref64(q, g, w):
    """fp64, from g: g_b, g_bias_b, g_bias_head (numpy)"""
    q, g, w = (torch.from_numpy(np.ascontiguousarray(t)).double() for t in (q, g, w))
    e = q[:, :, 1:-1, 1:-1]
    ge = fold(F.conv_transpose2d(g, w))
    g_b = torch.where(e <= 0, ge * (e + 1), ge)
    return g_b.numpy(), g_b.sum((0, 2, 3)).numpy(), g.sum().reshape(1).numpy()


def impulse_positions(H, W):
    """corners, the rows and columns next to a border (where the folds land), the edges of the 8 x 64 tiles, the middle"""
    rows = sorted({0, 1, H // 2, H - 2, H - 1, 7, 8} & set(range(H)))
    cols = sorted({0, 1, W // 2, W - 2, W - 1, 63, 64, 65} & set(range(W)))
    return [(i, j) for i in rows for j in cols]


def impulse_case(shape, pos):
    """one impulse of g at `pos` of the last image, weights of distinct integer codes, E > 0 -> q, g, w"""
    B, H, W = shape
    g = np.zeros((B, 1, H, W), np.float32)
    g[B - 1, 0, pos[0], pos[1]] = 1
    w = (1 + np.arange(C * 9, dtype=np.float32)).reshape(1, C, 3, 3)
    q = np.ones((B, C, H + 2, W + 2), np.float32)
    return q, g, w


def first_difference(got, want):
    """None, or a description of the first entry of got[B, C, H, W] that is not want"""
    bad = np.argwhere(got != want)
    if not len(bad):
        return None
    n, c, i, j = bad[0]
    return (f"{len(bad)} entries differ; first: image {n} channel {c} pixel ({i}, {j}) holds {got[n, c, i, j]} "
            f"for {want[n, c, i, j]} (weight codes are 1 + 9 c + 3 r + s)")
