"""Adam over every parameter tensor in ONE launch of libscsfm_opt.so (include/scsfm_opt.h; train.py --optimizer hip).

``Adam`` takes the constructor arguments of ``torch.optim.Adam`` -- parameter groups with their own ``lr``, ``betas``,
``eps`` and ``weight_decay`` -- and keeps its state flat: ``exp_avg`` and ``exp_avg_sq`` are two fp32 buffers over all
parameters of all groups, every tensor's segment on a 16-byte boundary, and the step counts are an int64 array on the host.
``step()`` writes one record per tensor (the parameter's and the gradient's address, the segment, and ``step_size`` and
``bias_correction2_sqrt`` computed in float64 from the tensor's OWN step count, as torch does) into a pinned table, uploads
it with one non-blocking copy and makes one library call on the current stream.  The chunk map behind the table is uploaded
again only when the set of tensors that have a gradient changed.  Nothing is read back.  A parameter whose ``.grad`` is
None is skipped and its step count does not advance, as under torch.  Groups that differ in ``betas`` or ``eps`` take one
launch each (train.py's two groups share them: one launch).

The order of the fp32 operations is the header's, one rounding per line, so a step can be restated in numpy bit for bit.
It is torch's formula (``lerp`` for the first moment) without the fused multiply-adds ATen's kernels contract to: results
agree with ``torch.optim.Adam`` to rounding, not bit for bit.

``state_dict()`` and ``load_state_dict()`` use ``torch.optim.Adam``'s layout -- ``state[i] = {'step', 'exp_avg',
'exp_avg_sq'}`` in the parameter's shape, tensors never stepped absent, ``param_groups`` as torch writes them -- so a file
written under either optimiser loads under the other.

Not supported, and refused: ``amsgrad``, ``maximize``, ``capturable``, ``differentiable``, ``decoupled_weight_decay``,
sparse gradients, parameters or gradients that are not contiguous fp32, parameters on more than one device, and HIP-graph
capture (the table is written on the host every step: ``step()`` raises when the current stream is capturing).
"""
from __future__ import annotations

import ctypes
import inspect

import numpy as np
import torch

from . import _lib, capi

CHUNK = 2048        # SCSFM_OPT_CHUNK
RECORD = np.dtype([("p", "<u8"), ("g", "<u8"), ("off", "<i8"), ("n", "<i4"), ("step_size", "<f4"), ("bc2_sqrt", "<f4"),
                   ("wd", "<f4")])
assert RECORD.itemsize == 40  # SCSFM_OPT_RECORD_BYTES
_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")


def _need_cuda(*ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("scsfm_hip.optim: parameters must live on a HIP device (torch 'cuda'); this package has no "
                               "CPU fallback")


def _torch_defaults():
    """torch.optim.Adam's own defaults, by name: ``param_groups`` then carries the keys the installed torch writes"""
    sig = inspect.signature(torch.optim.Adam.__init__)
    return {k: v.default for k, v in sig.parameters.items() if k not in ("self", "params")}


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **kwargs):
        defaults = _torch_defaults()
        unknown = set(kwargs) - set(defaults)
        if unknown:
            raise TypeError("unexpected arguments: {}".format(sorted(unknown)))
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kwargs)
        self._laid_out = False
        super().__init__(params, defaults)
        self._layout()

    # ------------------------------------------------------------------------------------------------ construction
    def add_param_group(self, param_group):
        if self._laid_out:
            raise RuntimeError("scsfm_hip.optim.Adam: the flat state is laid out at construction; groups cannot be added")
        super().add_param_group(param_group)

    @staticmethod
    def _check_group(group):
        for key in _UNSUPPORTED:
            if group.get(key, False):
                raise ValueError("scsfm_hip.optim.Adam does not support {}=True".format(key))
        if group.get("fused"):
            raise ValueError("scsfm_hip.optim.Adam does not support fused=True (that is ATen's kernel)")
        lr, (beta1, beta2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
        if any(isinstance(v, torch.Tensor) for v in (lr, beta1, beta2)):
            raise ValueError("scsfm_hip.optim.Adam takes lr and betas as Python numbers")
        if not (0.0 <= lr and 0.0 <= eps < float("inf") and 0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0 and 0.0 <= wd):
            raise ValueError("invalid lr / betas / eps / weight_decay: {} {} {} {}".format(lr, (beta1, beta2), eps, wd))

    def _layout(self):
        self._params = [p for group in self.param_groups for p in group["params"]]
        if not self._params:
            raise ValueError("optimizer got an empty parameter list")
        _need_cuda(*self._params)
        for group in self.param_groups:
            self._check_group(group)
        dev = self._params[0].device
        for p in self._params:
            if p.dtype != torch.float32 or p.is_sparse or not p.is_contiguous() or p.device != dev:
                raise ValueError("scsfm_hip.optim.Adam takes dense, contiguous fp32 parameters on one device; got {} {} on "
                                 "{}".format(p.dtype, tuple(p.shape), p.device))
        self._device = dev
        n = len(self._params)
        self._numel = np.array([p.numel() for p in self._params], np.int64)
        if int(self._numel.max()) >= 2 ** 31:
            raise ValueError("scsfm_hip.optim.Adam: a parameter of 2^31 or more elements")
        padded = (self._numel + 3) // 4 * 4                      # every segment starts on a 16-byte boundary
        self._offset = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
        total = max(int(padded.sum()), 4)
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        assert self.exp_avg.data_ptr() % 16 == 0 and self.exp_avg_sq.data_ptr() % 16 == 0
        self._steps = np.zeros(n, np.int64)
        self._group_of = np.repeat(np.arange(len(self.param_groups)), [len(g["params"]) for g in self.param_groups])
        # the whole chunk map, ordered by group (a launch covers a run of groups that share betas and eps)
        chunks = (self._numel + CHUNK - 1) // CHUNK
        tensor = np.repeat(np.arange(n, dtype=np.int32), chunks)
        first = np.repeat(np.cumsum(chunks) - chunks, chunks)
        self._full_map = np.stack([tensor, (np.arange(len(tensor)) - first).astype(np.int32)], axis=1)
        # one upload: the table, then on a 16-byte boundary the map
        self._table_bytes = (n * RECORD.itemsize + 15) // 16 * 16
        nbytes = self._table_bytes + max(len(tensor), 1) * 8
        pin = dev.type == "cuda"
        self._host = torch.zeros(nbytes, dtype=torch.uint8, pin_memory=pin)
        self._dev = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        assert self._dev.data_ptr() % 16 == 0
        raw = self._host.numpy()
        self._table = raw[:n * RECORD.itemsize].view(RECORD)
        self._map = raw[self._table_bytes:].view(np.int32).reshape(-1, 2)
        self._table["off"] = self._offset
        self._table["n"] = self._numel
        self._uploaded = None   # the gradient-presence mask the map on the device was built from
        self._launches = []     # (first entry, entries, beta1, beta2, eps) of the map on the device
        self._event = torch.cuda.Event() if pin else None
        self._laid_out = True

    def _segment(self, buf, i):
        return buf[int(self._offset[i]):int(self._offset[i] + self._numel[i])].view(self._params[i].shape)

    # ------------------------------------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None):
        """One Adam step of every parameter that has a gradient.  Not capturable into a HIP graph."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        dev = self._device
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("scsfm_hip.optim.Adam.step() writes its table on the host every step and cannot be captured "
                               "into a HIP graph")
        params = self._params
        n = len(params)
        grads = [p.grad for p in params]
        present = np.fromiter((g is not None for g in grads), bool, n)
        if not present.any():
            return loss
        for p, g in zip(params, grads):
            if g is not None and (g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.device != dev or
                                  g.numel() != p.numel()):
                raise RuntimeError("scsfm_hip.optim.Adam takes dense, contiguous fp32 gradients on the parameters' device; "
                                   "got {} {} for a parameter of shape {}".format(g.dtype, tuple(g.shape), tuple(p.shape)))
            if not p.is_contiguous():
                raise RuntimeError("scsfm_hip.optim.Adam: a parameter is no longer contiguous")
        for group in self.param_groups:  # (a scheduler, or the caller, may have changed them)
            self._check_group(group)
        # the per-tensor scalars, in float64 from each tensor's own count, as torch.optim.Adam computes them
        self._steps[present] += 1
        gi = self._group_of
        lr = np.array([g["lr"] for g in self.param_groups], np.float64)[gi]
        beta1 = np.array([g["betas"][0] for g in self.param_groups], np.float64)[gi]
        beta2 = np.array([g["betas"][1] for g in self.param_groups], np.float64)[gi]
        wd = np.array([g["weight_decay"] for g in self.param_groups], np.float64)[gi]
        t = np.maximum(self._steps, 1).astype(np.float64)  # (a tensor never stepped has no chunk: any finite value)
        step_size = lr / (1.0 - beta1 ** t)
        bc2_sqrt = (1.0 - beta2 ** t) ** 0.5
        if self._event is not None:
            self._event.synchronize()  # the previous step's upload has left the pinned buffer
        table = self._table
        table["p"] = np.fromiter((p.data_ptr() for p in params), np.uint64, n)
        table["g"] = np.fromiter((0 if g is None else g.data_ptr() for g in grads), np.uint64, n)
        table["step_size"] = step_size
        table["bc2_sqrt"] = bc2_sqrt
        table["wd"] = wd
        upto = self._table_bytes
        if self._uploaded is None or not np.array_equal(present, self._uploaded):
            upto = self._write_map(present)
        self._dev[:upto].copy_(self._host[:upto], non_blocking=True)
        if self._event is not None:
            self._event.record()
        lib = _lib.get_opt()
        base = self._dev.data_ptr()
        stream = ctypes.c_void_p(capi._stream(self._dev))
        for first, count, b1, b2, eps in self._launches:
            lib.call("scsfm_opt_adam_step_f32", ctypes.c_void_p(base), n,
                     ctypes.c_void_p(base + self._table_bytes + 8 * first), count, ctypes.c_void_p(self.exp_avg.data_ptr()),
                     ctypes.c_void_p(self.exp_avg_sq.data_ptr()), b1, b2, eps, stream)
        return loss

    def _write_map(self, present):
        """The map of the tensors that have a gradient into the pinned buffer -> the bytes to upload.  The entries of
        consecutive groups that share betas and eps form one launch."""
        keep = present[self._full_map[:, 0]]
        entries = self._full_map[keep]
        if len(entries) > len(self._map):
            raise RuntimeError("scsfm_hip.optim.Adam: the chunk map is longer than the buffer laid out for it")
        self._map[:len(entries)] = entries
        groups = self._group_of[entries[:, 0]]
        self._launches = []
        for k, group in enumerate(self.param_groups):
            count = int(np.count_nonzero(groups == k))
            if not count:
                continue
            first = int(np.argmax(groups == k))
            key = (float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]))
            if self._launches and self._launches[-1][2:] == key and sum(self._launches[-1][:2]) == first:
                self._launches[-1] = (self._launches[-1][0], self._launches[-1][1] + count) + key
            else:
                self._launches.append((first, count) + key)
        assert sum(c for _, c, *_ in self._launches) == len(entries)  # n_chunks IS the map's length
        self._uploaded = present.copy()
        return self._table_bytes + 8 * len(entries)

    # ------------------------------------------------------------------------------------------------ the state
    def state_dict(self):
        """torch.optim.Adam's layout: copies of the moments in the parameters' shapes, 'step' as torch's fp32 scalar."""
        state = {}
        for i in np.flatnonzero(self._steps > 0):
            i = int(i)
            state[i] = {"step": torch.tensor(float(self._steps[i]), dtype=torch.float32),
                        "exp_avg": self._segment(self.exp_avg, i).clone(),
                        "exp_avg_sq": self._segment(self.exp_avg_sq, i).clone()}
        groups, k = [], 0
        for group in self.param_groups:
            packed = {key: value for key, value in group.items() if key != "params"}
            packed["params"] = list(range(k, k + len(group["params"])))
            k += len(group["params"])
            groups.append(packed)
        return {"state": state, "param_groups": groups}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """A state dict of this class or of torch.optim.Adam over the same parameter lists."""
        groups = state_dict["param_groups"]
        if len(groups) != len(self.param_groups) or any(len(a["params"]) != len(b["params"])
                                                        for a, b in zip(groups, self.param_groups)):
            raise ValueError("loaded state dict has other parameter groups than the optimizer")
        ids = [i for g in groups for i in g["params"]]
        merged = []
        for saved, group in zip(groups, self.param_groups):
            new = {key: value for key, value in saved.items() if key != "params"}
            new["betas"] = tuple(new.get("betas", group["betas"]))
            merged.append({**group, **new, "params": group["params"]})
            self._check_group(merged[-1])
        staged = []
        for k, i in enumerate(ids):
            entry = state_dict["state"].get(i)
            if entry is None:
                staged.append(None)
                continue
            if "max_exp_avg_sq" in entry:
                raise ValueError("scsfm_hip.optim.Adam does not support amsgrad state")
            m, v = entry["exp_avg"], entry["exp_avg_sq"]
            if m.numel() != self._numel[k] or v.numel() != self._numel[k]:
                raise ValueError("loaded state of parameter {} has {} elements, the parameter {}".format(i, m.numel(),
                                                                                                        self._numel[k]))
            staged.append((int(round(float(entry["step"]))), m, v))
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self._steps[:] = 0
        for k, entry in enumerate(staged):
            if entry is not None:
                self._steps[k] = entry[0]
                self._segment(self.exp_avg, k).copy_(entry[1].reshape(self._params[k].shape))
                self._segment(self.exp_avg_sq, k).copy_(entry[2].reshape(self._params[k].shape))
        for group, new in zip(self.param_groups, merged):
            group.update(new)
        self._uploaded = None  # (betas or eps may have changed: the launches are formed again)
