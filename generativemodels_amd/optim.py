"""Adam / AdamW whose whole parameter update is one native launch (csrc/optim.hip), behind torch.optim's interface.

    opt = gm.optim.Adam(unet.parameters(), lr=2.5e-5)
    step = gm.GraphedForwardBackward(loss_fn, example_inputs, unet.parameters(), optimizer=opt)   # forward, loss, backward and update: one graph replay
    loss = step(x, t, eps)                                                                        # ... or, eagerly: loss.backward(); opt.step()

The kernel is driven by a descriptor table in device memory, one entry per chunk of a tensor (`plan_chunks`), so a step is one launch per parameter dtype
plus one tiny launch that advances the per-parameter step counters -- whatever the number of tensors.  The table is rebuilt and uploaded only when the set of
(parameter, gradient) addresses changes; the hyper-parameters live in a small device table, one fp64 row per param group, of which the host rewrites a row only
when a value has changed (torch's LR schedulers mutate `group["lr"]`); the step counters are device fp32 (torch's `capturable=True` convention).  `step()`
reads nothing back, so it can be captured into a HIP graph.

Subclasses of torch.optim.Optimizer with torch's constructor arguments, defaults, errors, `param_groups` keys and state layout: a checkpoint written by
torch.optim.Adam / AdamW resumes here and one written here resumes in torch.  Deviations: fp32 parameters take fp32 gradients and bf16 parameters bf16
gradients (any other pairing is a TypeError); the moments of bf16 parameters are kept in fp32 (torch keeps them in bf16); there is no CPU path."""
from __future__ import annotations

from collections import namedtuple
from itertools import chain
from typing import Iterable, List, Sequence

import torch
from torch import Tensor

__all__ = ["Adam", "AdamW", "plan_chunks", "Chunk", "CHUNK"]

ENTRY_WORDS = 8  # GM_OPTIM_ENTRY_WORDS
HYPER_DOUBLES = 8  # GM_OPTIM_HYPER_DOUBLES
# elements per table entry = per 256-thread work-group: 128 KiB of fp32 parameter.  A multiple of 8, so that a chunk's byte offset into its tensor is a multiple
# of 16 for 2- and 4-byte elements and the alignment of a chunk is the alignment of its tensor.  The C4 UNet's 41.7 M parameters make ~1400 work-groups.
CHUNK = 32768
_AMSGRAD, _MAXIMIZE, _DECOUPLED = 1, 2, 4

Chunk = namedtuple("Chunk", "tensor start count vec")


def plan_chunks(sizes: Sequence[int], addresses: Sequence[Sequence[int]], chunk: int = CHUNK) -> List[Chunk]:
    """Pure host planning of the descriptor table.  sizes[i]: elements of tensor i; addresses[i]: the byte addresses of its pointers (p, g, exp_avg,
    exp_avg_sq[, max_exp_avg_sq]).  -> one Chunk(tensor, start, count, vec) per table entry, in tensor order; every element of every tensor is in exactly one
    chunk, and `vec` (16-byte accesses) only where all of the tensor's pointers are 16-byte aligned -- a chunk starts a multiple of `chunk` elements into its
    tensor, which keeps that alignment.  An empty tensor has no chunk."""
    if chunk <= 0 or chunk % 8:
        raise ValueError("plan_chunks: the chunk size is a positive multiple of 8 elements")
    out = []
    for i, (n, addr) in enumerate(zip(sizes, addresses)):
        vec = all(a % 16 == 0 for a in addr)
        for start in range(0, int(n), chunk):
            out.append(Chunk(i, start, min(chunk, int(n) - start), vec))
    return out


def _scalar(x, what: str) -> float:
    if isinstance(x, Tensor):
        if x.numel() != 1:
            raise ValueError(f"Tensor {what} must be 1-element")
        return float(x)
    return x


class Adam(torch.optim.Optimizer):
    _decoupled_default = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False, decoupled_weight_decay=None):
        lr = _scalar(lr, "lr")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if not ((isinstance(betas[0], float) and isinstance(betas[1], float)) or (isinstance(betas[0], Tensor) and isinstance(betas[1], Tensor))):
            raise ValueError("betas must be either both floats or both Tensors")
        betas = (_scalar(betas[0], "betas[0]"), _scalar(betas[1], "betas[1]"))
        # torch's keys, so that a state dict moves both ways; foreach / capturable / differentiable / fused select among torch's implementations and mean nothing here
        defaults = {"lr": lr, "betas": betas, "eps": eps, "weight_decay": weight_decay, "amsgrad": amsgrad, "maximize": maximize, "foreach": None,
                    "capturable": False, "differentiable": False, "fused": None,
                    "decoupled_weight_decay": self._decoupled_default if decoupled_weight_decay is None else bool(decoupled_weight_decay)}
        super().__init__(params, defaults)
        self._steps = None  # fp32 device counters, one per parameter in param_groups order; state[p]["step"] is a view of its element
        self._key = None  # what the device table was built for: the (parameter, gradient) addresses
        self._tables = None  # (the page-locked staging buffer, the device buffer) of the live descriptor table
        self._spare = None  # a page-locked buffer of the live table's size, set aside by ensure_state() for a table built inside a capture
        self._launches: list = []  # (dtype code, byte offset of the dtype's entries in the device buffer, entries)
        self._active = (0, 0)  # (byte offset, count) of the counter indices the trailing launch advances
        self._updated: list = []  # the parameters the table updates: their version counters are bumped after every step
        self._hyper_dev = None
        self._hyper_rows: list = []
        self._frozen: list = []  # buffers a captured graph holds addresses of: kept alive, and never rewritten, as long as the optimizer lives

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            for k, v in self.defaults.items():
                group.setdefault(k, v)

    # ---- the per-step host work: no device synchronisation -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._plan():
            self._sync_hyper()
            self._launch()
        return loss

    def ensure_state(self) -> None:
        """Create the state of every parameter that holds a gradient now, without stepping (state cannot be created inside a stream capture: its zero
        fill would be replayed), and set aside the page-locked staging buffer that a table built inside a capture is uploaded from."""
        self._plan()
        if self._tables is not None:
            self._spare = torch.empty(self._tables[0].numel(), dtype=torch.int64).pin_memory()

    def _plan(self) -> bool:
        key: list = []
        for group in self.param_groups:
            key.append(group["amsgrad"])
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    try:
                        key.append(p.data_ptr())
                        key.append(g.data_ptr())
                    except Exception:  # (a sparse gradient has no data pointer: _rebuild names the parameter)
                        key.append(None)
        if key != self._key:
            self._rebuild()
            self._key = key
        return bool(self._launches)

    def _name(self, gi: int, j: int, p: Tensor) -> str:
        names = self.param_groups[gi].get("param_names")
        return f"parameter '{names[j]}'" if names else f"parameter {j} of param group {gi} (shape {tuple(p.shape)})"

    def _rebuild(self) -> None:
        import numpy as np

        from . import _native, ops

        todo, index, total = [], {}, 0
        for gi, group in enumerate(self.param_groups):
            for j, p in enumerate(group["params"]):
                index[p] = total
                total += 1
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse or g.layout != torch.strided:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                if (p.dtype, g.dtype) not in ((torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16)):
                    raise TypeError(f"gm.optim: {self._name(gi, j, p)} is {p.dtype} with a {g.dtype} gradient; fp32 parameters take fp32 gradients and bf16 "
                                    "parameters bf16 gradients")
                if p.layout != torch.strided or not p.is_contiguous() or not g.is_contiguous() or g.shape != p.shape:
                    raise ValueError(f"gm.optim: {self._name(gi, j, p)} or its gradient is not dense (contiguous, of the parameter's shape)")
                ops.require_device(p, g)
                todo.append((gi, p, g))
        capturing = bool(todo) and torch.cuda.is_current_stream_capturing()
        self._ensure_steps(total, index, todo[0][1].device if todo else None)
        per_dtype = {}
        self._updated = []
        active = []
        for gi, p, g in todo:
            st = self.state[p]
            ams = bool(self.param_groups[gi]["amsgrad"])
            if "exp_avg" not in st or (ams and "max_exp_avg_sq" not in st):
                if capturing:
                    raise RuntimeError("gm.optim: optimizer state cannot be created inside a stream capture (its zero fill would be replayed): run one eager "
                                       "step, or ensure_state() with the gradients in place, before capturing")
                st.setdefault("step", self._steps[index[p]])
                for name in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if ams else ()):
                    if name not in st:
                        st[name] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
            ptrs = [p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["max_exp_avg_sq"].data_ptr() if ams else 0]
            n, es = p.numel(), p.element_size()
            chunks = plan_chunks([n], [ptrs])
            if not chunks:
                continue
            ent = np.zeros((len(chunks), ENTRY_WORDS), dtype=np.int64)
            start = np.fromiter((c.start for c in chunks), dtype=np.int64, count=len(chunks))
            for k, (ptr, size) in enumerate(zip(ptrs, (es, es, 4, 4, 4))):
                ent[:, k] = ptr + start * size if ptr else 0
            ent[:, 5] = [c.count for c in chunks]
            ent[:, 6] = index[p]
            ent[:, 7] = gi | (int(chunks[0].vec) << 32)
            per_dtype.setdefault(ops.dt_code(p.dtype), []).append(ent)
            active.append(index[p])
            self._updated.append(p)
        self._launches = []
        if not per_dtype:
            self._tables = None
            return
        parts, words = [], 0
        for dt in sorted(per_dtype):
            ent = np.concatenate(per_dtype[dt])
            self._launches.append((dt, words * 8, len(ent)))
            parts.append(ent.reshape(-1))
            words += ent.size
        act = np.zeros((len(active) + 1) // 2 * 2, dtype=np.int32)
        act[:len(active)] = active
        self._active = (words * 8, len(active))
        parts.append(act.view(np.int64))
        flat = torch.from_numpy(np.concatenate(parts))
        if capturing:  # (page-locked memory cannot be allocated by a capturing thread: ensure_state() left a buffer of this table's size)
            if self._spare is None or self._spare.numel() < flat.numel():
                raise RuntimeError("gm.optim: the (parameter, gradient) set changed inside a stream capture and no staging buffer is at hand: call "
                                   "ensure_state() with gradients on the same parameters before capturing")
            host, self._spare = self._spare[:flat.numel()].copy_(flat), None
        else:
            host = flat.pin_memory()
        dev = torch.empty(host.shape, dtype=torch.int64, device=todo[0][1].device)  # (a new buffer every time: a captured graph may hold the old one's address)
        if capturing:  # a memcpy node that reads `host` at every replay
            _native.check(_native.lib().gm_optim_upload(dev.data_ptr(), host.data_ptr(), host.numel() * 8, ops._stream()), "gm_optim_upload")
        else:
            dev.copy_(host, non_blocking=True)
        self._tables = (host, dev)

    def _ensure_steps(self, total: int, index: dict, device) -> None:
        if self._steps is not None and self._steps.numel() >= total:
            return
        if device is None:
            return
        if self._frozen:
            raise RuntimeError("gm.optim: parameters cannot be added once a step has been captured into a graph (the graph holds the counters' address)")
        old = self._steps
        self._steps = torch.zeros(max(total, 1), dtype=torch.float32, device=device)
        if old is not None:
            self._steps[:old.numel()] = old
            for p, st in self.state.items():
                if "step" in st and p in index:
                    st["step"] = self._steps[index[p]]

    def _hyper_row(self, group) -> tuple:
        b1, b2 = group["betas"]
        flags = (_AMSGRAD if group["amsgrad"] else 0) | (_MAXIMIZE if group["maximize"] else 0) | (_DECOUPLED if group.get("decoupled_weight_decay") else 0)
        return (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), float(flags), 0.0, 0.0)

    def _sync_hyper(self) -> None:
        """Bring the device rows up to the param groups: an asynchronous copy from page-locked memory, on the current stream, of each row that changed."""
        rows = [self._hyper_row(g) for g in self.param_groups]
        if rows == self._hyper_rows:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("gm.optim: a hyper-parameter changed inside a stream capture; change param groups between replays and outside captures")
        if self._hyper_dev is None or self._hyper_dev.shape[0] < len(rows):
            if self._frozen:
                raise RuntimeError("gm.optim: param groups cannot be added once a step has been captured into a graph")
            self._hyper_dev = torch.empty((len(rows), HYPER_DOUBLES), dtype=torch.float64, device="cuda")
            self._hyper_rows = []
        for i, row in enumerate(rows):
            if i >= len(self._hyper_rows) or self._hyper_rows[i] != row:
                self._hyper_dev[i].copy_(torch.tensor(row, dtype=torch.float64).pin_memory(), non_blocking=True)
        self._hyper_rows = rows

    def _launch(self) -> None:
        from . import _native, ops

        lib, s = _native.lib(), ops._stream()
        host, dev = self._tables
        base = dev.data_ptr()
        for dt, off, n in self._launches:
            _native.check(lib.gm_adam_step(base + off, n, self._steps.data_ptr(), self._hyper_dev.data_ptr(), dt, s), "gm_adam_step")
        _native.check(lib.gm_adam_advance(self._steps.data_ptr(), base + self._active[0], self._active[1], s), "gm_adam_advance")
        if torch.cuda.is_current_stream_capturing():
            # the graph holds these addresses: keep the buffers, and build the next eager step's table elsewhere
            self._frozen.append((self._tables, self._steps, self._hyper_dev))
            self._key = None
        self._bump()

    def _bump(self) -> None:
        """A native write does not bump `param._version`, which every derived cache is keyed on (ops._cached: packed MFMA panels, fp32 copies; the graphed
        UNet's signature; the SPADE / rescaler caches): do it for every updated parameter -- host bookkeeping, no launch."""
        if self._updated:
            torch.autograd.graph.increment_version(self._updated)

    def _warm(self) -> None:
        """Run both kernels once on scratch tensors of every parameter dtype (a kernel's first launch loads its code object, which a capture must not do)."""
        import numpy as np

        from . import _native, ops

        self._sync_hyper()
        lib, s = _native.lib(), ops._stream()
        steps = torch.zeros(2, dtype=torch.float32, device="cuda")
        for dtype in sorted({p.dtype for g in self.param_groups for p in g["params"]}, key=str):
            p, g = torch.zeros(8, dtype=dtype, device="cuda"), torch.zeros(8, dtype=dtype, device="cuda")
            m, v = torch.zeros(8, dtype=torch.float32, device="cuda"), torch.zeros(8, dtype=torch.float32, device="cuda")
            ent = np.zeros(ENTRY_WORDS + 2, dtype=np.int64)
            ent[:ENTRY_WORDS] = [p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0, 8, 0, 1 << 32]
            dev = torch.from_numpy(ent).pin_memory().to("cuda", non_blocking=True)  # (words 8, 9: the counter list {0})
            _native.check(lib.gm_adam_step(dev.data_ptr(), 1, steps.data_ptr(), self._hyper_dev.data_ptr(), ops.dt_code(dtype), s), "gm_adam_step")
            _native.check(lib.gm_adam_advance(steps.data_ptr(), dev.data_ptr() + ENTRY_WORDS * 8, 1, s), "gm_adam_advance")

    # ---- checkpoints: torch's layout ------------------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        sd = super().state_dict()
        # (a counter is a view into the flat counter buffer: saved as a tensor of its own)
        sd["state"] = {k: {n: (v.clone() if n == "step" and isinstance(v, Tensor) else v) for n, v in st.items()} for k, st in sd["state"].items()}
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict) -> None:
        mine = {p: dict(st) for p, st in self.state.items()}  # tensors a captured graph may hold the addresses of: refilled in place
        super().load_state_dict(state_dict)
        # torch casts the moments to the parameter's dtype; here they are fp32 whatever it is: take them from the dict itself
        saved = dict(zip(chain.from_iterable(g["params"] for g in state_dict["param_groups"]), chain.from_iterable(g["params"] for g in self.param_groups)))
        index = {p: i for i, p in enumerate(chain.from_iterable(g["params"] for g in self.param_groups))}
        device = next((p.device for p in index), None)
        if self._steps is None or self._steps.numel() < len(index):
            self._ensure_steps(len(index), index, device)
        for k, src in state_dict["state"].items():
            p = saved.get(k)
            if p is None:
                continue
            st = self.state[p]
            for name in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
                if name in src:
                    have = mine.get(p, {}).get(name)
                    if have is not None and have.shape == src[name].shape and have.device == p.device:
                        st[name] = have.copy_(src[name])
                    else:
                        st[name] = src[name].detach().to(device=p.device, dtype=torch.float32, copy=True).contiguous()
            step = src.get("step", 0.0)
            self._steps[index[p]] = float(step)  # a host or a device tensor, or the plain number of old checkpoints
            st["step"] = self._steps[index[p]]
        self._key = None


class AdamW(Adam):
    _decoupled_default = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize)
