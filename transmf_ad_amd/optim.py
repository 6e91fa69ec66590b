"""Adam and SGD with the whole update of a parameter group in ONE launch, and the reference's `getOptimizer`.

Adam (csrc/adam.hip, tmf_adam_step) — reference: utils/utils.py:38-39 (getOptimizer -> torch.optim.Adam(net.parameters(),
lr=1e-4, betas default, weight decay 0)), stepped once per train step at kfold_train_adversarial.py:135.  Same constructor
arguments, update rule and skipping of parameters without a gradient as torch.optim.Adam (amsgrad / maximize / capturable /
foreach are not offered); the moment estimates of a parameter group live in two flat buffers, `state_dict()` exposes them per
parameter in torch's layout (`step`, `exp_avg`, `exp_avg_sq` views) so a checkpoint loads into torch.optim.Adam and back.

SGD (csrc/sgd.hip, tmf_sgd_step) — reference: utils/utils.py:34-37 (getOptimizer with --optimizer SGD: lr, weight_decay),
kfold_train_Mnet.py:85 (lr 0.001, momentum 0.9).  torch.optim.SGD's constructor order, weight decay and momentum
(dampening / nesterov / maximize are not offered: no reference caller uses them); the momentum buffers live in one flat
buffer and appear per parameter as `state[p]["momentum_buffer"]` views, only once the parameter has taken a step, as in torch.

getOptimizer(net_para, opt) — utils/utils.py:29-41: the optimizer `opt.optimizer` names plus its MultiStepLR.

Both classes read `group["lr"]` at every step (learning-rate schedulers work unchanged) and have no CPU path.
"""
import ctypes as C

import torch

from . import _lib


class _OneLaunch(torch.optim.Optimizer):
    """What both update rules need on the host: chunks of at most ADAM_MAX_TENSORS parameters (one launch each), their
    numel / pointer arrays and offsets in the flat state buffers, the gradient checks, and the rebuild of the kernel-side
    state after copy.deepcopy / pickle / load_state_dict (torch serialises only defaults, state and param_groups)."""

    def __setstate__(self, state):
        """copy.deepcopy / pickle: the kernel-side flat buffers and pointer tables are rebuilt from the per-parameter state
        (as after load_state_dict)."""
        super().__setstate__(state)
        self._rebuild_flat()

    def load_state_dict(self, state_dict):
        """torch's loader replaces the per-parameter state tensors: copy them back into the flat buffers the kernel uses."""
        super().load_state_dict(state_dict)
        self._rebuild_flat()

    def _group_state(self, group):
        """The group's chunks, made (by the subclass's _new_chunk) when the group is first stepped."""
        if getattr(self, "_flat", None) is None:
            self._flat = {}
        st = self._flat.get(id(group))
        if st is not None:
            return st
        ps = group["params"]
        if not ps:
            return None
        dev = ps[0].device
        for p in ps:
            if p.dtype != torch.float32 or p.device != dev or not p.is_cuda or not p.is_contiguous():
                raise _lib.TmfError(f"transmf_ad_amd.optim.{type(self).__name__}: parameters must be contiguous float32 tensors "
                                    "on one HIP device")
        chunks = []
        for s in range(0, len(ps), _lib.ADAM_MAX_TENSORS):
            sub = ps[s:s + _lib.ADAM_MAX_TENSORS]
            numel = (C.c_long * len(sub))(*[p.numel() for p in sub])
            total = _lib.query("tmf_adam_state_elems", len(sub), numel)
            off, offs = 0, []
            for p in sub:
                offs.append(off)
                off += (p.numel() + 3) & ~3
            pptr = (C.c_void_p * len(sub))(*[p.data_ptr() for p in sub])
            chunks.append(self._new_chunk(sub, numel, offs, pptr, total, dev))
        self._flat[id(group)] = chunks
        return chunks

    def _gradients(self, sub, pptr):
        """(the chunk's gradients, contiguous, None where a parameter has none; whether any is missing); refreshes the
        parameter pointers on the way."""
        grads = []
        missing = False
        for i, p in enumerate(sub):
            if p.data_ptr() != pptr[i]:
                pptr[i] = p.data_ptr()                      # parameter storage replaced (e.g. by .to())
            g = p.grad
            if g is None:
                grads.append(None)
                missing = True
                continue
            if g.is_sparse or g.dtype != torch.float32 or g.device != p.device:
                raise _lib.TmfError(f"transmf_ad_amd.optim.{type(self).__name__}: gradients must be dense float32 on the "
                                    "parameter's device")
            grads.append(g if g.is_contiguous() else g.contiguous())
        return grads, missing


class Adam(_OneLaunch):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError(f"invalid Adam hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self._flat = {}                      # id(group) -> (exp_avg, exp_avg_sq, offsets, numel array, param pointer array)

    def _new_chunk(self, sub, numel, offs, pptr, total, dev):
        m = torch.zeros(total, device=dev, dtype=torch.float32)
        v = torch.zeros(total, device=dev, dtype=torch.float32)
        # step counts as Python ints (no 156 x `.item()` per step): [0] = the count every parameter of the chunk shares,
        # [1] = {index: count} once some parameter sat out a step (torch's bias correction is per parameter), [2] = the
        # CPU tensor that every state[p]["step"] of the chunk IS while the counts agree (one add_ per step keeps torch's
        # state layout current); after a divergence each parameter gets a tensor of its own
        shared = torch.tensor(0.0)           # ONE `step` tensor for the whole chunk while the counts agree
        for p, o in zip(sub, offs):          # torch's per-parameter layout, as views of the flat buffers
            self.state[p] = {"step": shared, "exp_avg": m[o:o + p.numel()].view_as(p),
                             "exp_avg_sq": v[o:o + p.numel()].view_as(p)}
        return (sub, m, v, offs, numel, pptr, [0, None, shared])

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            chunks = self._group_state(group)
            if not chunks:
                continue
            b1, b2 = group["betas"]
            for sub, m, v, _offs, numel, pptr, cnt in chunks:
                grads, missing = self._gradients(sub, pptr)
                if not missing and cnt[1] is None:                   # every step of a normal run: ONE count for the chunk
                    cnt[0] += 1
                    cnt[2].add_(1.0)
                    steps = None
                    todo = (cnt[0],)
                else:                                                # some parameter sat out a step, now or earlier
                    if cnt[1] is None:
                        cnt[1] = {i: cnt[0] for i in range(len(sub))}
                        for p in sub:
                            self.state[p]["step"] = torch.tensor(float(cnt[0]))
                    for i, g in enumerate(grads):
                        if g is not None:
                            cnt[1][i] += 1
                            self.state[sub[i]]["step"] += 1
                    steps = [cnt[1][i] if g is not None else None for i, g in enumerate(grads)]
                    todo = sorted({s_ for s_ in steps if s_ is not None})
                # one launch per distinct step count (one, unless some parameter sat out earlier steps)
                for step in todo:
                    gptr = (C.c_void_p * len(sub))(*[g.data_ptr() if (g is not None and (steps is None or steps[i] == step))
                                                     else None for i, g in enumerate(grads)])
                    with torch.cuda.device(m.device):
                        _lib.call("tmf_adam_step", len(sub), pptr, gptr, numel, m.data_ptr(), v.data_ptr(), float(group["lr"]),
                                  float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), step,
                                  torch.cuda.current_stream().cuda_stream)
        return loss

    def _rebuild_flat(self):
        self._flat = {}
        loaded = {p: dict(st) for p, st in self.state.items()}
        if not loaded:
            return
        for group in self.param_groups:
            for sub, m, v, offs, _numel, _pptr, cnt in self._group_state(group) or ():
                counts = []
                for p, o in zip(sub, offs):
                    old = loaded.get(p)
                    n = 0
                    if old and "exp_avg" in old:
                        m[o:o + p.numel()].copy_(old["exp_avg"].reshape(-1))
                        v[o:o + p.numel()].copy_(old["exp_avg_sq"].reshape(-1))
                        n = int(float(old.get("step", 0.0)))
                        self.state[p]["step"] = torch.tensor(float(n))
                    counts.append(n)
                if len(set(counts)) <= 1:
                    cnt[0], cnt[1] = (counts[0] if counts else 0), None
                    cnt[2].fill_(float(cnt[0]))
                    for p in sub:
                        self.state[p]["step"] = cnt[2]
                else:
                    cnt[0], cnt[1] = max(counts), dict(enumerate(counts))
                    # diverged counts: EVERY parameter gets a step tensor of its own (one that loaded no state would otherwise keep
                    # the chunk's shared tensor, and step() would advance it once per such parameter)
                    for p, n in zip(sub, counts):
                        self.state[p]["step"] = torch.tensor(float(n))


class _SgdChunk:
    """One launch's worth of parameters: the arrays of _OneLaunch._group_state, the flat momentum buffer (allocated at the
    first step that has a momentum) and the per-parameter "no buffer yet" flags tmf_sgd_step takes."""
    __slots__ = ("sub", "numel", "offs", "pptr", "total", "dev", "buf", "fresh", "nfresh")

    def __init__(self, sub, numel, offs, pptr, total, dev):
        self.sub, self.numel, self.offs, self.pptr, self.total, self.dev = sub, numel, offs, pptr, total, dev
        self.buf = None
        self.fresh = (C.c_int * len(sub))(*([1] * len(sub)))
        self.nfresh = len(sub)

    def view(self, i):
        p, o = self.sub[i], self.offs[i]
        return self.buf[o:o + p.numel()].view_as(p)

    def need_buf(self):
        if self.buf is None:
            # no fill: a parameter's slice is written (buf = g') before the kernel ever reads it
            self.buf = torch.empty(self.total, device=self.dev, dtype=torch.float32)


class SGD(_OneLaunch):
    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError(f"invalid SGD hyper-parameters lr={lr} momentum={momentum} weight_decay={weight_decay}")
        extras = dict(dampening=(dampening, 0), nesterov=(nesterov, False), maximize=(maximize, False), foreach=(foreach, None),
                      differentiable=(differentiable, False), fused=(fused, None))
        asked = [f"{k}={v!r}" for k, (v, default) in extras.items() if v != default]
        if asked:
            raise ValueError(f"transmf_ad_amd.optim.SGD does not offer {', '.join(asked)}: use torch.optim.SGD for that")
        # dampening and nesterov stay in the groups (at their only values) so that state_dict() loads into torch.optim.SGD
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False))
        self._flat = {}                      # id(group) -> [_SgdChunk]

    def _new_chunk(self, sub, numel, offs, pptr, total, dev):
        return _SgdChunk(sub, numel, offs, pptr, total, dev)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            if group.get("dampening", 0) != 0 or group.get("nesterov") or group.get("maximize"):     # e.g. a loaded state dict
                raise ValueError("transmf_ad_amd.optim.SGD does not offer dampening, nesterov or maximize: use "
                                 "torch.optim.SGD for that")
            mom = float(group["momentum"])
            for ch in self._group_state(group) or ():
                grads, _missing = self._gradients(ch.sub, ch.pptr)
                if ch.total == 0:
                    continue
                if mom != 0:
                    ch.need_buf()
                gptr = (C.c_void_p * len(ch.sub))(*[None if g is None else g.data_ptr() for g in grads])
                with torch.cuda.device(ch.dev):
                    # fresh and seasoned parameters go in the same launch: the flags ride in the kernel's tensor table
                    _lib.call("tmf_sgd_step", len(ch.sub), ch.pptr, gptr, ch.numel, ch.buf.data_ptr() if mom != 0 else None,
                              ch.fresh if mom != 0 else None, float(group["lr"]), mom, float(group["weight_decay"]),
                              torch.cuda.current_stream().cuda_stream)
                if mom != 0 and ch.nfresh:
                    for i, g in enumerate(grads):
                        if g is not None and ch.fresh[i]:            # first participation: the buffer now holds g'
                            ch.fresh[i] = 0
                            ch.nfresh -= 1
                            self.state[ch.sub[i]]["momentum_buffer"] = ch.view(i)
        return loss

    def _rebuild_flat(self):
        self._flat = {}
        loaded = {p: st.get("momentum_buffer") for p, st in self.state.items()}
        if all(b is None for b in loaded.values()):
            return                           # nothing stepped with a momentum yet: no device is touched
        for group in self.param_groups:
            for ch in self._group_state(group) or ():
                for i, p in enumerate(ch.sub):
                    old = loaded.get(p)
                    if old is None:          # no buffer yet (torch: absent or None): stays fresh
                        continue
                    ch.need_buf()
                    view = ch.view(i)
                    view.copy_(old)
                    self.state[p]["momentum_buffer"] = view
                    ch.fresh[i] = 0
                    ch.nfresh -= 1


def getOptimizer(net_para, opt):
    """The reference's utils.getOptimizer on this package's optimizers: (optimizer, MultiStepLR) for opt.optimizer 'SGD'
    (milestones 10 and 26) or 'Adam' (25 and 36), gamma 0.1, with opt.lr and opt.weight_decay; None for any other name, as
    the reference returns.  net_para: an iterable of parameters, e.g. the generator net.parameters()."""
    recipe = {"SGD": (SGD, [10, 26]), "Adam": (Adam, [25, 36])}.get(opt.optimizer)
    if recipe is None:
        return None
    cls, milestones = recipe
    optimizer = cls(net_para, lr=opt.lr, weight_decay=opt.weight_decay)
    return optimizer, torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=milestones, gamma=0.1)
