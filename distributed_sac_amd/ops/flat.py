"""Flat parameter/gradient storage + fused Adam.

MI355X-first design decision: every optimizer group's parameters live as
views into ONE contiguous fp32 buffer, with gradients accumulating into a
matching flat buffer.  Consequences:

- the optimizer step is ONE multi-element HIP kernel (``adam_step_``) instead
  of the reference's per-tensor torch.optim.Adam loop (K9 in SURVEY §2.6);
- the Polyak target update is ONE kernel over the flat pair (K10);
- data-parallel gradient all-reduce is ONE RCCL message per group over xGMI
  (latency-dominated at these sizes — SURVEY §2.7 MI355X mapping).

``FusedAdam`` emits/consumes ``torch.optim.Adam``-format state dicts so
reference checkpoints (learner.save_checkpoint) round-trip.
"""

from __future__ import annotations

import math
from typing import Dict, Iterable, List, Optional

import torch
import torch.nn as nn

from . import has_native, native, native_enabled, torch_ref


def _flatten_into(params: List[torch.Tensor]) -> torch.Tensor:
    numel = sum(p.numel() for p in params)
    if numel == 0:
        return torch.empty(0)
    flat = torch.empty(numel, dtype=torch.float32, device=params[0].device)
    off = 0
    for p in params:
        n = p.numel()
        flat[off:off + n].copy_(p.detach().reshape(-1))
        off += n
    return flat


class FlatParams:
    """Re-homes a list of nn.Parameters into one flat fp32 buffer.

    After construction each parameter's ``.data`` is a view of
    :attr:`flat_data` and its ``.grad`` a view of :attr:`flat_grad`;
    autograd accumulates straight into the flat gradient.
    """

    def __init__(self, params: Iterable[nn.Parameter], with_grad: bool = True):
        self.params: List[nn.Parameter] = [p for p in params]
        assert len(self.params) > 0, "empty parameter group"
        dev = self.params[0].device
        for p in self.params:
            assert p.device == dev, "all group params must share a device"
            assert p.dtype == torch.float32, "flat groups are fp32"
        self.flat_data = _flatten_into([p.data for p in self.params])
        self.flat_grad = (torch.zeros_like(self.flat_data) if with_grad else None)
        off = 0
        self.offsets: List[int] = []
        for p in self.params:
            n = p.numel()
            self.offsets.append(off)
            p.data = self.flat_data[off:off + n].view_as(p.data)
            if with_grad:
                p.grad = self.flat_grad[off:off + n].view_as(p.data)
            off += n
        self.numel = off

    def zero_grad(self) -> None:
        if self.flat_grad is not None:
            self.flat_grad.zero_()

    def adopt_grad_arena(self, arena: torch.Tensor, offset: int) -> int:
        """Re-home this group's flat gradient into a shared arena slice so
        several groups can all-reduce as ONE message.  Returns the next
        free arena offset."""
        n = self.numel
        new = arena[offset:offset + n]
        if self.flat_grad is not None:
            new.copy_(self.flat_grad)
        self.flat_grad = new
        self.rebind_grads()
        return offset + n

    def rebind_grads(self) -> None:
        """Re-point .grad views (autograd can replace .grad if it was None)."""
        for p, off in zip(self.params, self.offsets):
            g = self.flat_grad[off:off + p.numel()].view_as(p.data)
            if p.grad is not g:
                p.grad = g

    def view_like(self, p: nn.Parameter) -> torch.Tensor:
        i = self.params.index(p)
        off = self.offsets[i]
        return self.flat_data[off:off + p.numel()].view_as(p.data)


@torch.no_grad()
def polyak_flat_(t: torch.Tensor, s: torch.Tensor, tau: float,
                 mirror: Optional[torch.Tensor] = None) -> None:
    """t <- tau*s + (1-tau)*t over two flat fp32 tensors (whole buffers or
    matching slices); with ``mirror`` set, t's bf16 compute mirror is
    refreshed in the same kernel (no separate cast launch)."""
    if t.is_cuda and native_enabled() and has_native():
        native().polyak_(t, s, float(tau), mirror)
        return
    t.mul_(1.0 - tau).add_(s, alpha=tau)
    if mirror is not None:
        mirror.copy_(t)


def flat_polyak_(target: FlatParams, source: FlatParams, tau: float,
                 mirror: Optional[torch.Tensor] = None) -> None:
    """:func:`polyak_flat_` over whole groups.  Requires identical
    parameter ordering (enforced by matching numel)."""
    assert target.numel == source.numel
    polyak_flat_(target.flat_data, source.flat_data, tau, mirror)


def _native_step(opts: List["FusedAdam"], rng_bump, pre_prologed, arena0,
                 polyak) -> None:
    """The one caller of the HIP steppers: <= 3 optimizers with device
    state and the same betas/eps, see :meth:`FusedAdam.step_many`."""
    clip = opts[0].max_grad_norm is not None
    assert all((o.max_grad_norm is not None) == clip for o in opts), \
        "clipping is per launch: set it on every optimizer"
    args = [
        [o.group.flat_data for o in opts],
        [o.group.flat_grad for o in opts],
        [o.exp_avg for o in opts],
        [o.exp_avg_sq for o in opts],
        [o._dev_state for o in opts],
        [o.lr for o in opts],
        opts[0].betas[0], opts[0].betas[1], opts[0].eps,
        [o.bf16_mirror if o.bf16_mirror is not None
         else torch.Tensor() for o in opts]]
    if clip:
        args += [opts[0]._clip_slots,
                 [o.max_grad_norm for o in opts],
                 [o._clip_state for o in opts],
                 [o._skips for o in opts]]
    args += [rng_bump, 1 if pre_prologed else 0,
             arena0[0] if arena0 is not None else None,
             int(arena0[1]) if arena0 is not None else 0]
    if polyak is not None:
        target, source, tau, mirror = polyak
        assert target.numel == source.numel
        args += [target.flat_data, source.flat_data, float(tau), mirror]
    ext = native()
    (ext.adam_step_clip_ if clip else ext.adam_step_multi_)(*args)


class FusedAdam:
    """Adam over a FlatParams group as one fused kernel.

    Matches torch.optim.Adam numerics exactly (bias-corrected, eps outside
    the sqrt of the bias-corrected v — torch default, weight_decay=0) and
    speaks torch.optim.Adam state_dict format for checkpoint compatibility
    with the reference (learner.save_checkpoint stores
    ``optimizer.state_dict()``).
    """

    def __init__(self, group: FlatParams, lr: float,
                 betas=(0.9, 0.999), eps: float = 1e-8, ref_params=None,
                 max_grad_norm: Optional[float] = None):
        self.group = group
        # (de)serialization order: the reference checkpoints index optimizer
        # state by the REFERENCE's parameter order (e.g. chain(critic1,
        # critic2)), which may differ from the flat group's layout (we
        # interleave layer pairs for the stacked twin-GEMM views).
        self.ref_params = (list(ref_params) if ref_params is not None
                           else list(group.params))
        self._ref_offsets = []
        for rp in self.ref_params:
            i = next(j for j, q in enumerate(group.params) if q is rp)
            self._ref_offsets.append(group.offsets[i])
        self.lr = float(lr)
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self._step_count = 0
        self.exp_avg = torch.zeros_like(group.flat_data)
        self.exp_avg_sq = torch.zeros_like(group.flat_data)
        # hipGraph-capturable path: the step counter + bias-correction
        # coefficients live on-device ({step, step_size, inv_sqrt_bc2}) so a
        # captured update keeps correct Adam bias correction across replays.
        self._dev_state = None
        # optional bf16 compute mirror refreshed in the SAME adam kernel
        # (set by the engine when mixed precision is on)
        self.bf16_mirror: Optional[torch.Tensor] = None
        if group.flat_data.is_cuda and native_enabled() and has_native():
            self._dev_state = torch.zeros(3, device=group.flat_data.device)
        # gradient-norm clipping (None = off): fp32 {norm, coef, s} of the
        # last step, the int32 skip counter and, for the HIP path, the
        # sum-of-squares partial slots (3 ranges x 256 blocks)
        self.max_grad_norm: Optional[float] = None
        self._clip_state: Optional[torch.Tensor] = None
        self._skips: Optional[torch.Tensor] = None
        self._clip_slots: Optional[torch.Tensor] = None
        self.set_max_grad_norm(max_grad_norm)

    def set_max_grad_norm(self, max_grad_norm: Optional[float],
                          skips: Optional[torch.Tensor] = None) -> None:
        """Clip this group's gradient to a global L2 norm of
        ``max_grad_norm`` inside :meth:`step` / :meth:`step_many` and skip
        the step when the norm is not finite (``inf``: guard only; ``None``:
        off).  The flat gradient itself stays unclipped.  A skipped step
        still advances the step counter: bias correction counts ATTEMPTED
        steps.  ``skips``: int32 [1] counter to bump instead of this
        optimizer's own, so several optimizers can share one."""
        self.max_grad_norm = torch_ref.check_max_grad_norm(max_grad_norm)
        if self.max_grad_norm is None:
            return
        dev = self.group.flat_data.device
        if self._clip_state is None:
            self._clip_state = torch.tensor([0.0, 1.0, 0.0], device=dev)
            self._skips = torch.zeros(1, dtype=torch.int32, device=dev)
            if self._dev_state is not None:
                self._clip_slots = torch.zeros(3 * 256, device=dev)
        if skips is not None:
            assert skips.dtype == torch.int32 and skips.device == dev
            self._skips = skips

    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        """L2 norm of the last step's unclipped gradient (0-d view)."""
        return None if self._clip_state is None else self._clip_state[0]

    @property
    def clip_coef(self) -> Optional[torch.Tensor]:
        """Factor the last step applied (1 = unclipped, 0 = skipped)."""
        return None if self._clip_state is None else self._clip_state[1]

    @property
    def grad_skips(self) -> Optional[torch.Tensor]:
        """Cumulative number of skipped steps (0-d int32 view)."""
        return None if self._skips is None else self._skips[0]

    @property
    def step_count(self) -> int:
        if self._dev_state is not None:
            return int(self._dev_state[0].item())
        return self._step_count

    @step_count.setter
    def step_count(self, v: int) -> None:
        self._step_count = int(v)
        if self._dev_state is not None:
            with torch.no_grad():
                self._dev_state[0] = float(v)

    def zero_grad(self) -> None:
        self.group.zero_grad()

    @torch.no_grad()
    def step(self, pre_prologed: bool = False, arena=None) -> None:
        """arena: optional ``(tensor [>=S, numel], S)`` of split-K gradient
        partials — the Adam kernel sums them (s order, as reduce_arena),
        writes the sum to the flat gradient and steps, in one launch."""
        p, g = self.group.flat_data, self.group.flat_grad
        m, v = self.exp_avg, self.exp_avg_sq
        b1, b2 = self.betas
        if self._dev_state is not None:
            _native_step([self], None, pre_prologed, arena, None)
            return
        if arena is not None:
            g.zero_()
            for s in range(int(arena[1])):
                g.add_(arena[0][s])
        self._step_count += 1
        if self.max_grad_norm is not None:
            sq, norm, coef, ok = torch_ref.grad_clip_coef(
                g, self.max_grad_norm)
            self._clip_state.copy_(torch.stack([norm, coef, sq]))
            if not bool(ok):
                self._skips.add_(1)
                return
            g = g * coef   # the flat gradient stays unclipped
        bc1 = 1 - b1 ** self._step_count
        bc2 = 1 - b2 ** self._step_count
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = (v.sqrt() / math.sqrt(bc2)).add_(self.eps)
        p.addcdiv_(m, denom, value=-self.lr / bc1)

    @staticmethod
    @torch.no_grad()
    def step_many(opts: List["FusedAdam"], rng_bump=None,
                  pre_prologed: bool = False, arena0=None,
                  polyak=None) -> None:
        """Step up to 3 optimizers in ONE fused kernel launch (same betas/
        eps; device-resident step state required).  rng_bump: optional
        int64 counter the prolog kernel increments once — the per-update
        bump for the counter-based device RNG (race-free: the prolog is a
        single-block kernel and every RNG consumer runs in other
        launches); with ``pre_prologed`` the caller's prolog has bumped it
        already.

        arena0: optional ``(tensor [>=S, numel], S)`` split-K partials of
        the FIRST optimizer's gradient, summed inside the same launch (see
        :meth:`step`).  polyak: optional ``(target, source, tau, mirror)``
        — ``flat_polyak_(target, source, tau, mirror)`` done by the same
        launch; ``source`` must not be one of ``opts``' groups."""
        live = [o for o in opts if o is not None]
        assert arena0 is None or (opts and opts[0] is not None), \
            "arena0 belongs to the first optimizer"
        if (1 <= len(live) <= 3
                and all(o._dev_state is not None for o in live)
                and all(o.betas == live[0].betas and o.eps == live[0].eps
                        for o in live)):
            _native_step(live, rng_bump, pre_prologed, arena0, polyak)
            return
        # unfused fallback: same effects, one launch each
        if rng_bump is not None and not pre_prologed:
            rng_bump.add_(1)
        for j, o in enumerate(live):
            o.step(pre_prologed=pre_prologed,
                   arena=arena0 if (j == 0 and o is opts[0]) else None)
        if polyak is not None:
            flat_polyak_(*polyak)

    # -- torch.optim.Adam-compatible (de)serialization ---------------------

    def state_dict(self) -> Dict:
        state = {}
        for i, (p, off) in enumerate(zip(self.ref_params, self._ref_offsets)):
            n = p.numel()
            state[i] = {
                "step": torch.tensor(float(self.step_count)),
                "exp_avg": self.exp_avg[off:off + n].view_as(p.data).clone(),
                "exp_avg_sq": self.exp_avg_sq[off:off + n].view_as(p.data).clone(),
            }
        group = {
            "lr": self.lr, "betas": self.betas, "eps": self.eps,
            "weight_decay": 0, "amsgrad": False, "maximize": False,
            "foreach": None, "capturable": False, "differentiable": False,
            "fused": None, "params": list(range(len(self.ref_params))),
        }
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd: Dict) -> None:
        groups = sd["param_groups"]
        assert len(groups) == 1, "FusedAdam holds one param group"
        g0 = groups[0]
        self.lr = float(g0.get("lr", self.lr))
        if "betas" in g0:
            self.betas = tuple(float(b) for b in g0["betas"])
        self.eps = float(g0.get("eps", self.eps))
        state = sd["state"]
        if not state:
            return
        steps = []
        for i, (p, off) in enumerate(zip(self.ref_params, self._ref_offsets)):
            key = i if i in state else str(i)
            if key not in state:
                continue
            st = state[key]
            n = p.numel()
            self.exp_avg[off:off + n].copy_(
                st["exp_avg"].reshape(-1).to(self.exp_avg.device))
            self.exp_avg_sq[off:off + n].copy_(
                st["exp_avg_sq"].reshape(-1).to(self.exp_avg_sq.device))
            s = st["step"]
            steps.append(int(s.item() if torch.is_tensor(s) else s))
        if steps:
            self.step_count = max(steps)
