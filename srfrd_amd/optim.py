"""`srfrd_amd.Adam`: torch.optim.Adam's update (reference trainer.py:390: ``Adam(model.parameters(), lr, betas=(0.9, 0.98))``)
for the module-level drop-in path, stepped by ONE launch over the model's flat parameter vector.

The reference loop (trainer.py:29-41) stays as it is - ``model(...)`` -> BCE -> ``loss.backward()`` -> ``optimizer.step()`` - only
the optimizer's constructor changes.  Every parameter of a srfrd_amd module is a view of one fp32 vector
``[item table | pad | dense]`` and the backward op returns every gradient as a view of one flat gradient vector, so the step
is ``srfrd_adam_step`` over the whole vector (same arithmetic as the fused trainer's tail; torch's foreach Adam walks 31
tensors with a handful of launches each and costs more host time than the model's kernels take).

That one in-place launch is taken when the list holds every parameter of the module, all with a gradient of the same step
count, laid out as views of one gradient vector.  Otherwise the gradients are gathered into a flat buffer (gradient
accumulation over several backward calls, hooks that replace them), and what must not move - tensors left out of the list
(frozen), listed ones without a gradient (torch skips them) - is copied aside before the launch and back after it, so it
comes out bit-unchanged: a parameter and its two moments per held tensor and step, i.e. three copies of the item table per
step when the table is frozen (0.6 GB of traffic at 1 M x 50).  Like torch, every parameter keeps its own step count (the
bias corrections follow it); parameters whose counts differ are stepped by one launch per count.  ``state_dict()`` /
``load_state_dict()`` use torch.optim.Adam's own format, so a run can move between the two optimizers (and
``FusedTrainer``).

`srfrd_amd.AdamW` is the same optimizer with torch.optim.AdamW's decoupled weight decay: it steps through ``srfrd_adamw_step``
behind ``srfrd_step_begin_sched`` at the group's current ``lr`` (a constant schedule: torch's LR schedulers keep working, they
rewrite ``lr`` between steps)."""
from __future__ import annotations

import torch

from . import _lib
from ._lib import call


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False):
        if weight_decay != 0.0 or amsgrad:
            raise ValueError("srfrd_amd.Adam implements plain Adam (the reference's optimizer): no weight decay / amsgrad")
        super().__init__(params, dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps)))
        if len(self.param_groups) != 1:
            raise ValueError("srfrd_amd.Adam takes ONE parameter group: model.parameters() of one srfrd_amd module")
        self._flat = self._m = self._v = self._gbuf = self._dev_state = None
        self._spans = None
        self._full = False          # the list holds every parameter of the module that owns the vector (set by _resolve)
        self._loaded = None         # load_state_dict's state, scattered into _m / _v / _counts by the next _resolve
        self._counts = [0] * len(self.param_groups[0]["params"])     # torch's per-parameter "step"
        self._p0 = self._pl = None
        self._steps = 0             # the step count the device state holds (its word 0)

    # ---- the flat vector behind the parameters -------------------------------------------------------------------------
    def _resolve(self):
        from .modules import flat_owner
        ps = self.param_groups[0]["params"]
        st = ps[0].untyped_storage()
        base = st.data_ptr()
        if any(p.untyped_storage().data_ptr() != base or p.dtype != torch.float32 or not p.is_contiguous() for p in ps):
            raise RuntimeError("srfrd_amd.Adam steps the flat parameter vector of a srfrd_amd module: run one forward first (the "
                               "parameters become views of it then), and pass model.parameters() of ONE model")
        spans = sorted((p.storage_offset(), p.numel()) for p in ps)
        n = (spans[-1][0] + spans[-1][1] + 3) // 4 * 4
        flat = torch.empty(0, device=ps[0].device, dtype=torch.float32).set_(st, 0, (n,))
        if self._flat is None or self._flat.data_ptr() != flat.data_ptr() or self._flat.numel() != n:
            dev = flat.device
            self._flat = flat
            m_old, v_old = self._m, self._v
            self._m = torch.zeros(n, device=dev, dtype=torch.float32)
            self._v = torch.zeros(n, device=dev, dtype=torch.float32)
            if m_old is not None and m_old.numel() == n:      # (the model re-flattened, e.g. moved: keep the moments)
                self._m.copy_(m_old); self._v.copy_(v_old)
            self._gbuf = None
            self._dev_state = torch.zeros(32, device=dev, dtype=torch.int32)
            self._dev_state[0] = self._steps
        self._spans = [(p, p.storage_offset(), p.numel()) for p in ps]
        # Whether one launch over [0, n) steps nothing but the listed tensors: the list must hold every parameter of the module
        # whose flat vector this is (the gaps left are its alignment padding, which stays zero).  Dense tensors are packed
        # with no alignment, so a frozen one may share a float4 with a listed one, at the tail as anywhere else.
        owner = flat_owner(base)
        listed = set(spans)
        self._full = owner is not None and all((off, q.numel()) in listed for q, off in owner._slots)
        if self._loaded is not None:
            loaded, self._loaded = self._loaded, None
            self._m.zero_(); self._v.zero_()
            self._counts = [0] * len(ps)
            for i, (p, off, k) in enumerate(self._spans):
                s = loaded.get(i)
                if s is not None:
                    self._m[off:off + k] = s["exp_avg"].to(device=p.device, dtype=torch.float32).reshape(-1)
                    self._v[off:off + k] = s["exp_avg_sq"].to(device=p.device, dtype=torch.float32).reshape(-1)
                    self._counts[i] = int(float(s["step"]))

    def _flat_grad(self, in_place_ok):
        """the gradients as one vector aligned with the flat parameters: in place when they already are views of one and
        the launch may read all of [0, n) from there (in_place_ok: every parameter of the module is stepped)"""
        base = last = None
        for p, off, n in (self._spans if in_place_ok else ()):
            g = p.grad
            if g is None or not g.is_contiguous():
                base = None
                break
            b = g.data_ptr() - 4 * off
            if base is None:
                base = b
            elif b != base:
                base = None
                break
            last = g
        if base is not None and last.dtype == torch.float32 and last.device == self._flat.device:
            # (one dtype / device test: tensors laid out at the parameters' own offsets of one buffer are views of one vector)
            st = last.untyped_storage()
            if st.data_ptr() <= base and base + 4 * self._flat.numel() <= st.data_ptr() + st.nbytes():
                return base, last          # (the vector's address; keep a reference alive until the launch is enqueued)
        if self._gbuf is None:
            self._gbuf = torch.zeros_like(self._flat)
        for p, off, n in self._spans:
            if p.grad is None:
                self._gbuf[off:off + n].zero_()
            else:
                self._gbuf[off:off + n].copy_(p.grad.reshape(-1))
        return self._gbuf, self._gbuf

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ps = self.param_groups[0]["params"]
        if all(p.grad is None for p in ps):
            return loss
        if ps[0].device.type != "cuda":
            raise RuntimeError("srfrd_amd.Adam runs on the ROCm GPU only (no CPU fallback)")
        if self._spans is None or ps[0].data_ptr() != self._p0 or ps[-1].data_ptr() != self._pl:
            self._resolve()             # (first step, or the model re-flattened its parameters)
            self._p0, self._pl = ps[0].data_ptr(), ps[-1].data_ptr()
        g = self.param_groups[0]
        groups = {}                     # step count -> the listed parameters with a gradient that have taken that many steps
        for i, (p, off, k) in enumerate(self._spans):
            if p.grad is not None:
                groups.setdefault(self._counts[i], []).append((off, k))
        gptr, keep = self._flat_grad(self._full and len(groups) == 1 and sum(map(len, groups.values())) == len(ps))
        n = self._flat.numel()
        for count, spans in sorted(groups.items()):
            # Each launch steps all of [0, n).  Off the in-place path, what it must not step - parameters left out of the
            # list, listed ones without a gradient or of another step count - is saved here and put back after it: the
            # kernel's slices start on multiples of 4, parameters do not, so it cannot be launched per span.
            held = []
            if keep is self._gbuf:
                lo = 0
                for off, k in sorted(spans) + [(n, 0)]:
                    if off > lo:
                        held.append((lo, off, self._flat[lo:off].clone(), self._m[lo:off].clone(), self._v[lo:off].clone()))
                    lo = max(lo, off + k)
            if count != self._steps:
                self._dev_state[0] = count
            # t += 1 and the bias corrections in double precision on the device, then the step over the whole vector
            self._launch(gptr, n, g)
            self._steps = count + 1
            for lo, hi, p, m, v in held:
                self._flat[lo:hi].copy_(p); self._m[lo:hi].copy_(m); self._v[lo:hi].copy_(v)
        for i, (p, _, _) in enumerate(self._spans):
            if p.grad is not None:
                self._counts[i] += 1
        del keep
        return loss

    def _vector(self, gptr, n, g):
        """what both Adam entry points take of this optimizer: the whole flat vector, no loss statistics, no bf16 shadow"""
        return dict(param=self._flat, grad=gptr, m=self._m, v=self._v, n=n, i0=0, i1=n, n_zero=0, beta1=g["betas"][0],
                    beta2=g["betas"][1], eps=g["eps"], state=self._dev_state, stats=None, table_bf16=None, n_table=0)

    def _launch(self, gptr, n, g):
        call("srfrd_step_begin", state=self._dev_state, lr=g["lr"], beta1=g["betas"][0], beta2=g["betas"][1])
        call("srfrd_adam_step", **self._vector(gptr, n, g))

    def _decay_of(self, g):
        """what state_dict()'s param group says about the decay"""
        return {}

    def _check_loaded_group(self, group):
        if any(group.get(k) for k in ("weight_decay", "amsgrad", "maximize")):
            raise ValueError("srfrd_amd.Adam implements plain Adam (no weight decay / amsgrad / maximize)")

    # ---- torch.optim.Adam's state format ---------------------------------------------------------------------------------
    def state_dict(self):
        g = self.param_groups[0]
        ps = g["params"]
        state = {}
        if self._loaded is not None:                   # loaded before the parameters were resolved: hand it back as it came
            state = {i: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in s.items()} for i, s in self._loaded.items()}
        elif self._spans is not None:
            for i, (p, off, n) in enumerate(self._spans):
                if self._counts[i] > 0:                # (torch holds state only for parameters it has stepped)
                    state[i] = {"step": torch.tensor(float(self._counts[i])),
                                "exp_avg": self._m[off:off + n].view(p.shape).clone(),
                                "exp_avg_sq": self._v[off:off + n].view(p.shape).clone()}
        group = {"lr": g["lr"], "betas": g["betas"], "eps": g["eps"], "weight_decay": 0, "amsgrad": False, "maximize": False,
                 "foreach": None, "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": False,
                 "params": list(range(len(ps)))}
        group.update(self._decay_of(g))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        group = sd["param_groups"][0]
        self._check_loaded_group(group)
        g = self.param_groups[0]
        g["lr"], g["betas"], g["eps"] = float(group["lr"]), (float(group["betas"][0]), float(group["betas"][1])), float(group["eps"])
        # Kept until the next _resolve() scatters it into the moments: the parameters become views of the flat vector only
        # at the model's first forward, so a state loaded right after construction (the usual resume order) must wait.
        self._loaded = {int(i): {"step": s["step"], "exp_avg": s["exp_avg"].detach().clone(), "exp_avg_sq": s["exp_avg_sq"].detach().clone()}
                        for i, s in sd["state"].items()}
        self._spans = None


class AdamW(Adam):
    """``srfrd_amd.Adam`` with torch.optim.AdamW's decoupled weight decay: ``p *= 1 - lr * weight_decay`` ahead of the Adam
    update, over the whole flat vector as one group (``srfrd_adamw_step``)."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False):
        if amsgrad:
            raise ValueError("srfrd_amd.AdamW: no amsgrad")
        if not (float(weight_decay) >= 0.0) or float(weight_decay) == float("inf"):
            raise ValueError(f"weight_decay must be finite and >= 0 (got {weight_decay})")
        super().__init__(params, lr, betas, eps)
        self.param_groups[0]["weight_decay"] = float(weight_decay)

    def _launch(self, gptr, n, g):
        # a constant schedule at the group's CURRENT rate: state[4] = lr / bc1, state[7] = 1 - lr * weight_decay
        opts = _lib.OptimOpts(float(g["lr"]), g["betas"][0], g["betas"][1], float(g["weight_decay"]), 0.0, 0, 0,
                              _lib.SCHEDULES["constant"], 0)
        call("srfrd_step_begin_sched", state=self._dev_state, opts=opts)
        call("srfrd_adamw_step", **self._vector(gptr, n, g), clip=None)

    def _decay_of(self, g):
        return {"weight_decay": g["weight_decay"], "decoupled_weight_decay": True}

    def _check_loaded_group(self, group):
        if any(group.get(k) for k in ("amsgrad", "maximize")):
            raise ValueError("srfrd_amd.AdamW: no amsgrad / maximize")
        if group.get("weight_decay") and group.get("decoupled_weight_decay") is False:
            raise ValueError("srfrd_amd.AdamW implements decoupled weight decay only: this state was saved under the coupled, "
                             "L2-style weight_decay of torch.optim.Adam")

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self.param_groups[0]["weight_decay"] = float(sd["param_groups"][0].get("weight_decay") or 0.0)
