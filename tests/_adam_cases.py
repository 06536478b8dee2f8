"""The cases of the one-launch Adam (include/scsfm_opt.h), shared by tests/test_opt_hostsim.py (the kernel compiled for
the host simulator) and tests/test_gpu_optimizer.py (libscsfm_opt.so on the device), and the numpy restatement of the
header that both compare with, bit for bit.

A case lays its tensors out in four arenas of fp32 -- parameters, gradients, exp_avg, exp_avg_sq -- that are pre-filled
with a sentinel bit pattern; the expected arenas are the same arrays with the numpy step applied to the tensors' segments,
so comparing whole arenas also shows that nothing was written outside a segment.  A backend moves arenas to where the
library can reach them (host memory for the simulator, the device for the GPU).  Test infrastructure only."""
from __future__ import annotations

import ctypes

import numpy as np

f32 = np.float32
CHUNK = 2048
SENTINEL = 0x7FC0DEAD   # a NaN no step computes
GUARD = 64              # floats between two tensors of an arena, and at its ends
RECORD = np.dtype([("p", "<u8"), ("g", "<u8"), ("off", "<i8"), ("n", "<i4"), ("step_size", "<f4"), ("bc2_sqrt", "<f4"),
                   ("wd", "<f4")])
SIZES = (1, 3, 4, 5, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
BETAS, EPS = (0.9, 0.999), 1e-8
LRS = (1e-3, 3e-2)      # two groups
STEPS = 5
ABSENT_IN = (2, 4)      # the steps (from 1) in which the lagging tensor has no gradient


def numpy_step(p, g, m, v, step_size, bc2_sqrt, wd, beta1=BETAS[0], beta2=BETAS[1], eps=EPS):
    """The header's lines on fp32 arrays, one rounding each -> (p, m, v).  step_size, bc2_sqrt, wd: np.float32."""
    assert all(a.dtype == f32 for a in (p, g, m, v)) and all(type(s) is f32 for s in (step_size, bc2_sqrt, wd))
    b1c, b2, b2c, e = f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(eps)
    with np.errstate(all="ignore"):
        if wd != 0:
            t = wd * p
            g = g + t
        t = g - m
        t = b1c * t
        m = m + t
        a = v * b2
        t = b2c * g
        t = t * g
        v = a + t
        d = np.sqrt(v)
        d = d / bc2_sqrt
        d = d + e
        t = m / d
        t = step_size * t
        p = p - t
    assert p.dtype == f32 and m.dtype == f32 and v.dtype == f32
    return p, m, v


def host_scalars(lr, step, beta1=BETAS[0], beta2=BETAS[1]):
    """torch.optim.Adam's two scalars of a tensor at its step count ``step``, in Python floats, rounded to fp32"""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return f32(lr / bias_correction1), f32(bias_correction2 ** 0.5)


class Tensor:
    def __init__(self, n, shifted, kind, group, lagging=False):
        self.n, self.shifted, self.kind, self.group, self.lagging = n, shifted, kind, group, lagging
        self.step = 0


def default_tensors():
    """Every size of SIZES once with all four addresses 16-byte aligned and once with the parameter and the gradient one
    element past such an address; the groups alternate; gradients that are exactly 0, of magnitude 1e-22 (the
    second moment underflows to 0 or to its smallest subnormals), of magnitude 1e-20 (it is subnormal) and of magnitude 1e18
    in both layouts; one aligned tensor of 257 lags."""
    out = []
    for shifted in (False, True):
        for k, n in enumerate(SIZES):
            out.append(Tensor(n, shifted, "normal", k % 2))
        for k, kind in enumerate(("zero", "tiny", "small", "huge")):
            out.append(Tensor(CHUNK + 5, shifted, kind, k % 2))
    out.append(Tensor(257, False, "normal", 1, lagging=True))
    return out


def smoke_tensors():
    """__graft_entry__._smoke_opt's four shapes"""
    return [Tensor(n, False, "normal", k % 2) for k, n in enumerate((7, 4 * 6, 2 * CHUNK + 3, 3 * 5 * 5))]


def gradient(rng, t):
    g = rng.standard_normal(t.n).astype(f32)
    if t.kind == "zero":
        g[:] = 0
    elif t.kind == "tiny":
        g *= f32(1e-22)
    elif t.kind == "small":
        g *= f32(1e-20)
    elif t.kind == "huge":
        g *= f32(1e18)
    return g


def _arena(tensors, shift_ok):
    """-> (element count, [first element of every tensor]): tensors GUARD apart, starts on multiples of 4 elements, one
    element further on for a shifted tensor (where the arena takes part in the shift)"""
    starts, at = [], GUARD
    for t in tensors:
        at = (at + 3) // 4 * 4
        starts.append(at + (1 if shift_ok and t.shifted else 0))
        at = starts[-1] + t.n + GUARD
    return at, starts


class HostBackend:
    """arenas in host memory on 64-byte boundaries (the simulator's library takes HOST pointers)"""
    stream = None

    def upload(self, a):
        raw = np.empty(a.nbytes + 64, np.uint8)
        skip = -raw.ctypes.data % 64
        view = raw[skip:skip + a.nbytes].view(a.dtype).reshape(a.shape)
        view[...] = a
        return view

    def write(self, h, a):
        h[...] = a

    def ptr(self, h):
        return h.ctypes.data

    def download(self, h):
        return h.copy()


def run_case(lib, backend, tensors, wd, seed=0, steps=STEPS, absent_in=ABSENT_IN):
    """``steps`` steps of the library on the case's arenas, each compared with the numpy restatement bit for bit, arenas
    whole.  -> the step counts."""
    rng = np.random.default_rng(seed)
    n_p, at_p = _arena(tensors, True)       # parameters and gradients: shifted tensors start one element on
    n_s = int(sum((t.n + 3) // 4 * 4 for t in tensors))
    off = np.concatenate([[0], np.cumsum([(t.n + 3) // 4 * 4 for t in tensors])[:-1]]).astype(np.int64)
    sent = np.array([SENTINEL], np.int32).view(f32)[0]
    P = np.full(n_p, sent, f32)
    G = np.full(n_p, sent, f32)
    M = np.full(n_s + 2 * GUARD, sent, f32)  # the flat buffers: handed over GUARD elements in
    V = np.full(n_s + 2 * GUARD, sent, f32)
    for t, a, o in zip(tensors, at_p, off):
        P[a:a + t.n] = rng.standard_normal(t.n).astype(f32)
        M[GUARD + o:GUARD + o + t.n] = 0
        V[GUARD + o:GUARD + o + t.n] = 0
    hP, hG, hM, hV = (backend.upload(a) for a in (P, G, M, V))
    n = len(tensors)
    table = np.zeros(n, RECORD)
    table["p"] = [backend.ptr(hP) + 4 * a for a in at_p]
    table["off"] = off
    table["n"] = [t.n for t in tensors]
    table["wd"] = wd
    for t, a in zip(tensors, at_p):  # the layout is what it says
        assert (backend.ptr(hP) + 4 * a) % 16 == (4 if t.shifted else 0)
    assert (backend.ptr(hM) + 4 * GUARD) % 16 == 0 and (backend.ptr(hV) + 4 * GUARD) % 16 == 0
    for s in range(1, steps + 1):
        G[...] = sent
        present = [not (t.lagging and s in absent_in) for t in tensors]
        for t, a, ok in zip(tensors, at_p, present):
            if ok:
                G[a:a + t.n] = gradient(rng, t)
                t.step += 1
        backend.write(hG, G)
        scal = [host_scalars(LRS[t.group], max(t.step, 1)) for t in tensors]
        table["g"] = [backend.ptr(hG) + 4 * a if ok else 0 for a, ok in zip(at_p, present)]
        table["step_size"] = [x[0] for x in scal]
        table["bc2_sqrt"] = [x[1] for x in scal]
        entries = np.array([(k, c) for k, (t, ok) in enumerate(zip(tensors, present)) if ok
                            for c in range((t.n + CHUNK - 1) // CHUNK)], np.int32).reshape(-1, 2)
        hT, hC = backend.upload(table.view(np.uint8)), backend.upload(entries)
        lib.call("scsfm_opt_adam_step_f32", ctypes.c_void_p(backend.ptr(hT)), n, ctypes.c_void_p(backend.ptr(hC)),
                 len(entries), ctypes.c_void_p(backend.ptr(hM) + 4 * GUARD), ctypes.c_void_p(backend.ptr(hV) + 4 * GUARD),
                 BETAS[0], BETAS[1], EPS, backend.stream)
        for t, a, o, ok, (step_size, bc2_sqrt) in zip(tensors, at_p, off, present, scal):
            if not ok:
                continue  # its parameter and its state keep their bits
            sl, st = slice(a, a + t.n), slice(GUARD + o, GUARD + o + t.n)
            P[sl], M[st], V[st] = numpy_step(P[sl], G[sl], M[st], V[st], step_size, bc2_sqrt, f32(wd))
        for name, h, want in (("param", hP, P), ("grad", hG, G), ("exp_avg", hM, M), ("exp_avg_sq", hV, V)):
            got = backend.download(h)
            bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
            assert bad.size == 0, f"step {s}, {name}: {bad.size} words differ, first at {bad[0]}: " \
                                  f"{got[bad[0]]!r} for {want[bad[0]]!r}"
    return [t.step for t in tensors]
