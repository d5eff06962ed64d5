"""SACEngine — the learner's update step for all variants.

Implements the exact update math of the reference learners:

- 'sac' / 'vsac' (LunarLander_Distributed_SAC/src/learner.py:203-239,
  MT1_Distributed_VSAC/src/learner.py): LL-style actor, two separate
  critics + two targets, scalar log_alpha, H_bar = -action_dim.
- 'mtsac' (MT10_Distributed_MTSAC/src/learner.py:253-325): MT-style actor,
  one twin-Q critic + target, per-task log_alpha vector, per-sample alpha
  gather, optional task-weighted losses.
- 'care' lives in :mod:`.care` (adds the context/state encoder machinery).

MI355X-first mechanics under the reference math:

- every optimizer group's params/grads live in ONE flat fp32 buffer
  (:class:`~distributed_sac_amd.ops.flat.FlatParams`), so Adam is one fused
  kernel, the Polyak target update is one kernel, and data-parallel gradient
  all-reduce is one RCCL message per group;
- forward/backward run through the fused HIP MLP + squashed-Gaussian ops;
- the whole update is hipGraph-capturable (fixed shapes, graph-safe RNG) —
  see :meth:`SACEngine.maybe_capture`.
"""

from __future__ import annotations

import os
from typing import Dict, Optional

import torch
import torch.nn as nn

from ..config import SACConfig
from ..models import Actor, Critic, LLActor, LLCritic
from ..ops import functional as Fops
from ..ops.chain import ManualChain, forward_pair, pack_chains
from ..ops.flat import FlatParams, FusedAdam, flat_polyak_


class SACEngine:
    """Holds models/optimizers and performs one SAC gradient update."""

    def __init__(self, cfg: SACConfig, device: torch.device | str = "cpu",
                 precision: Optional[str] = None,
                 max_grad_norm: Optional[float] = None):
        self.precision = (precision or
                          os.environ.get("DSAC_PRECISION", "fp32"))
        self.cfg = cfg
        self.variant = cfg.variant
        self.device = torch.device(device)
        self.gamma = cfg.gamma
        self.tau = cfg.tau
        self.reward_scale = cfg.reward_scale
        self.use_weighted_loss = cfg.use_weighted_loss and cfg.variant == "mtsac"
        # strict-parity mode reproducing the reference's degenerate
        # (B,)x(B,1)->(B,B) weighted-loss broadcast (docs/PARITY.md);
        # supported on the torch path only — the fused HIP kernels
        # implement the corrected per-sample weighting
        self.degenerate_w = \
            getattr(cfg, "weighted_loss_mode", "corrected") == "reference"
        self.num_tasks = cfg.num_tasks if cfg.variant in ("mtsac", "care") else 1
        self.update_iteration = 0
        self.total_step = 0
        self._graph = None
        self._eps_queue: Optional[list] = None  # test hook: deterministic eps
        self.ddp = None  # optional DataParallelGroup (set via attach_ddp)
        # prioritized replay: the attached replay (attach_per) and what the
        # last prioritized update left for the write-back
        self._per = None
        self.per_indices: Optional[torch.Tensor] = None
        self.per_new_priorities: Optional[torch.Tensor] = None
        self._per_zeroed = False
        # optional state: the bf16 / CARE / capture setup below fills in
        # what its path has, every reader sees a plain attribute
        self._bf16 = False
        self._se_fast = False
        self._rng_ctr: Optional[torch.Tensor] = None
        self._target_bf16: Optional[torch.Tensor] = None
        self._ctx_chain = None
        self._dw_arenas: dict = {}
        self._graph_chunk = 1
        self._dp_graphs = None
        self.context_encoder_optimizer = None
        self._build_models()
        self._build_optimizers()
        self._init_grad_clip(max_grad_norm)

    def _init_grad_clip(self, max_grad_norm: Optional[float]) -> None:
        """Opt-in gradient-norm clipping: the argument, else the cfg's
        ``max_grad_norm``, else ``DSAC_MAX_GRAD_NORM``, else off.  Critic,
        actor and (CARE) context encoder are clipped each on its own norm,
        as ``clip_grad_norm_`` per optimizer; alpha is guarded only.  All
        groups bump ONE skip counter, the ``grad_skips`` metric."""
        from ..ops.torch_ref import check_max_grad_norm
        c = check_max_grad_norm(max_grad_norm)
        if c is None:
            c = self.cfg.max_grad_norm_choice
        self.max_grad_norm = c
        if c is None:
            return
        self._grad_skips = torch.zeros(1, dtype=torch.int32,
                                       device=self.device)
        self.critic_optimizer.set_max_grad_norm(c, self._grad_skips)
        self.actor_optimizer.set_max_grad_norm(c, self._grad_skips)
        self.log_alpha_optimizer.set_max_grad_norm(float("inf"),
                                                   self._grad_skips)
        ctx = self.context_encoder_optimizer
        if ctx is not None:
            ctx.set_max_grad_norm(c, self._grad_skips)

    def _clip_metrics(self, out: Dict[str, torch.Tensor]):
        """With clipping on, add the groups' gradient norms (of the
        unclipped, all-reduced gradient) and the cumulative skip count:
        views of device state the steps refresh in place."""
        if self.max_grad_norm is None:
            return out
        out["critic_grad_norm"] = self.critic_optimizer.grad_norm
        out["actor_grad_norm"] = self.actor_optimizer.grad_norm
        ctx = self.context_encoder_optimizer
        if ctx is not None:
            out["context_grad_norm"] = ctx.grad_norm
        out["grad_skips"] = self._grad_skips[0]
        return out

    def _next_eps(self, like: torch.Tensor) -> torch.Tensor:
        if self._eps_queue:
            return self._eps_queue.pop(0).to(like.device)
        return torch.randn_like(like)

    def _eps_cat(self, mu: torch.Tensor, B: int,
                 in_kernel: bool = False) -> torch.Tensor:
        """eps for the batched [next | current] actor pass ``mu [2B, A]``:
        two queued draws (test hook), else storage the squash kernel fills
        from the counter RNG (``in_kernel``), else one randn launch."""
        if self._eps_queue:
            return torch.cat([self._next_eps(mu[:B]), self._next_eps(mu[:B])])
        if in_kernel:
            return torch.empty(mu.shape, device=mu.device, dtype=mu.dtype)
        return torch.randn_like(mu)

    def _sample(self, states: torch.Tensor):
        """Actor sampling with squashed-Gaussian op (both actor families)."""
        mu, log_std_raw = self.actor(states)
        eps = self._next_eps(mu)
        return Fops.squashed_gaussian(mu, log_std_raw, eps, self.actor.k)

    # ------------------------------------------------------------------
    def _build_models(self) -> None:
        cfg, dev = self.cfg, self.device
        if self.variant in ("sac", "vsac"):
            self.actor = LLActor(cfg.state_dim, cfg.action_dim,
                                 cfg.actor_hidden_dim, cfg.action_bound).to(dev)
            self.local_critic_1 = LLCritic(cfg.state_dim, cfg.action_dim,
                                           cfg.critic_hidden_dim).to(dev)
            self.local_critic_2 = LLCritic(cfg.state_dim, cfg.action_dim,
                                           cfg.critic_hidden_dim).to(dev)
            self.target_critic_1 = LLCritic(cfg.state_dim, cfg.action_dim,
                                            cfg.critic_hidden_dim).to(dev)
            self.target_critic_2 = LLCritic(cfg.state_dim, cfg.action_dim,
                                            cfg.critic_hidden_dim).to(dev)
            self.log_alpha = nn.Parameter(torch.tensor(
                [float(cfg.log_alpha)], device=dev))
        elif self.variant == "mtsac":
            self.actor = Actor(cfg.state_dim, cfg.action_dim,
                               cfg.actor_hidden_dim, cfg.action_bound,
                               num_tasks=cfg.num_tasks).to(dev)
            self.local_critic = Critic(cfg.state_dim, cfg.action_dim,
                                       cfg.critic_hidden_dim,
                                       num_tasks=cfg.num_tasks).to(dev)
            self.target_critic = Critic(cfg.state_dim, cfg.action_dim,
                                        cfg.critic_hidden_dim,
                                        num_tasks=cfg.num_tasks).to(dev)
            # per-task log_alpha (reference MT10…MTSAC/src/learner.py:115-121)
            self.log_alpha = nn.Parameter(torch.full(
                (cfg.num_tasks,), float(cfg.log_alpha), device=dev))
        else:
            raise ValueError(f"variant {self.variant} not handled here")
        self.H_bar = torch.tensor([-float(cfg.action_dim)], device=dev)
        self.H_bar_f = -float(cfg.action_dim)  # python scalar: graph-safe
        self.alpha = self.log_alpha.exp().detach()

    @staticmethod
    def _critic_linears(c1_or_critic, c2=None):
        """Per-layer Linear pairs (Q1_i, Q2_i) across both critic styles."""
        if c2 is not None:  # LL style: two modules
            l1 = [c1_or_critic.first_layer] + list(c1_or_critic.layer_module)
            l2 = [c2.first_layer] + list(c2.layer_module)
        else:  # MT style: one module with Q_function_1/2 Sequentials
            l1 = [m for m in c1_or_critic.Q_function_1 if isinstance(m, nn.Linear)]
            l2 = [m for m in c1_or_critic.Q_function_2 if isinstance(m, nn.Linear)]
        return list(zip(l1, l2))

    def _critic_layer_pairs(self, target: bool = False):
        if self.variant in ("sac", "vsac"):
            a = self.target_critic_1 if target else self.local_critic_1
            b = self.target_critic_2 if target else self.local_critic_2
            return self._critic_linears(a, b)
        return self._critic_linears(self.target_critic if target
                                    else self.local_critic)

    def _critic_params(self):
        """Interleaved per-layer order [Q1.w_i, Q2.w_i, Q1.b_i, Q2.b_i] so
        the flat buffer contains contiguous stacked [2,N,K] weights for the
        grouped twin-GEMM kernels."""
        out = []
        for l1, l2 in self._critic_layer_pairs():
            out += [l1.weight, l2.weight, l1.bias, l2.bias]
        return out

    def _target_params(self):
        out = []
        for l1, l2 in self._critic_layer_pairs(target=True):
            out += [l1.weight, l2.weight, l1.bias, l2.bias]
        return out

    def _build_twin_stacks(self, group, pairs, with_grad: bool):
        """Stacked [2,N,K]/[2,N] leaf views into a flat buffer, with .grad
        views into the flat gradient so autograd accumulates straight into
        the all-reduce/Adam buffer."""
        ws, bs = [], []
        for l1, l2 in pairs:
            for (pa, pb, shape, dest) in (
                    (l1.weight, l2.weight, l1.weight.shape, ws),
                    (l1.bias, l2.bias, l1.bias.shape, bs)):
                ia = next(i for i, q in enumerate(group.params) if q is pa)
                ib = next(i for i, q in enumerate(group.params) if q is pb)
                off = group.offsets[ia]
                n = pa.numel()
                assert group.offsets[ib] == off + n, "stacking needs adjacency"
                view = group.flat_data[off:off + 2 * n].view(2, *shape)
                stack = view.detach()
                if with_grad:
                    stack.requires_grad_(True)
                    stack.grad = group.flat_grad[off:off + 2 * n].view(2, *shape)
                dest.append(stack)
        return ws, bs

    def _build_optimizers(self) -> None:
        cfg = self.cfg
        self.actor_group = FlatParams(self.actor.parameters())
        self.critic_group = FlatParams(self._critic_params())
        self.target_group = FlatParams(self._target_params(), with_grad=False)
        self.alpha_group = FlatParams([self.log_alpha])
        self.actor_optimizer = FusedAdam(self.actor_group, lr=cfg.lr_actor)
        # checkpoint state is indexed in the REFERENCE optimizer order:
        # chain(critic1, critic2) for LL/VSAC (learner.build_optimizer),
        # local_critic.parameters() for MT — not our interleaved layout
        if self.variant in ("sac", "vsac"):
            ref_order = (list(self.local_critic_1.parameters())
                         + list(self.local_critic_2.parameters()))
        else:
            ref_order = list(self.local_critic.parameters())
        self.critic_optimizer = FusedAdam(self.critic_group,
                                          lr=cfg.lr_critic,
                                          ref_params=ref_order)
        # reference uses lr_actor for log_alpha (learner.py build_optimizer)
        self.log_alpha_optimizer = FusedAdam(self.alpha_group, lr=cfg.lr_actor)
        self._twin_local = self._build_twin_stacks(
            self.critic_group, self._critic_layer_pairs(), with_grad=True)
        self._twin_target = self._build_twin_stacks(
            self.target_group, self._critic_layer_pairs(target=True),
            with_grad=False)
        # frozen aliases of the local critic stacks (same storage, no
        # requires_grad): the actor pass needs dQ/d(action) but the critic
        # weight grads it would deposit are discarded (reference zeroes them
        # next update) — skipping their computation saves 4 dW GEMMs/step.
        self._twin_local_frozen = ([w.detach() for w in self._twin_local[0]],
                                   [b.detach() for b in self._twin_local[1]])
        # actor+alpha share one gradient arena: their all-reduce (both due
        # between the same backward and the fused Adam) is ONE RCCL message
        self._aa_arena = torch.zeros(
            self.actor_group.numel + self.alpha_group.numel,
            device=self.device)
        off = self.actor_group.adopt_grad_arena(self._aa_arena, 0)
        self.alpha_group.adopt_grad_arena(self._aa_arena, off)
        self._init_bf16_mirrors()
        self.hard_copy_targets()

    # -- bf16 mixed precision: fp32 masters + bf16 compute mirrors --------
    def _init_bf16_mirrors(self) -> None:
        self._bf16 = (self.precision == "bf16"
                      and self.device.type == "cuda")
        if not self._bf16:
            return
        dev = self.device
        # persistent zero-initialized workspace for the one-launch loss
        # reductions (per-block partial slots + self-resetting ticket)
        self._loss_ws = torch.zeros(256, device=dev)
        self._aloss_ws = torch.zeros(256, device=dev)
        # same for the fixed-order alpha-gradient reduction of
        # actor_alpha_loss_bwd2: ticket + (batch blocks x tasks) slots;
        # a batch too large for it takes the kernel's one-block path
        self._dla_ws = torch.zeros(2048, device=dev)
        # the fused actor/alpha fwd+bwd kernel: one ticket, 32x4 metric
        # slots, then up to 32 blocks x 32 tasks of alpha-gradient slots
        self._aafb_ws = torch.zeros(1 + 32 * 4 + 32 * 32, device=dev)
        # persistent counter for the in-kernel RNG, seeded from the torch
        # seed so runs stay reproducible end-to-end
        self._rng_ctr = torch.tensor(
            [int(torch.initial_seed()) & 0x7FFFFFFF],
            dtype=torch.int64, device=dev)
        self._critic_bf16 = torch.empty(self.critic_group.numel,
                                        dtype=torch.bfloat16, device=dev)
        self._target_bf16 = torch.empty(self.target_group.numel,
                                        dtype=torch.bfloat16, device=dev)
        self._actor_bf16 = torch.empty(self.actor_group.numel,
                                       dtype=torch.bfloat16, device=dev)
        self._twin_local_bf16 = self._stack_views(self.critic_group,
                                                  self._critic_bf16,
                                                  self._critic_layer_pairs())
        self.critic_optimizer.bf16_mirror = self._critic_bf16
        self.actor_optimizer.bf16_mirror = self._actor_bf16
        ws, bs = self._actor_weights()
        self._actor_ws_bf16 = self._mirror_views(self.actor_group,
                                                 self._actor_bf16, ws)
        # the manual update's chains; their fragment-packed weights are
        # re-packed per update (pre-step sets in seg1, the post-Adam
        # critic in seg2)
        pairs = self._critic_layer_pairs()
        self._critic_chain = ManualChain(
            self._twin_local_bf16, self._twin_local[1], G=2,
            group=self.critic_group,
            w_params=[l1.weight for l1, _ in pairs],
            b_params=[l1.bias for l1, _ in pairs])
        self._target_chain = ManualChain(
            self._stack_views(self.target_group, self._target_bf16,
                              self._critic_layer_pairs(target=True)),
            self._twin_target[1], G=2, dx=False)
        self._actor_chain = ManualChain(
            self._actor_ws_bf16, bs, group=self.actor_group,
            w_params=ws, b_params=bs)
        self.refresh_bf16()

    @staticmethod
    def _mirror_views(group, mirror, ws):
        """bf16 mirror views shaped like the fp32 weights ``ws``."""
        offs = [group.offsets[next(j for j, q in enumerate(group.params)
                                   if q is w)] for w in ws]
        return [mirror[off:off + w.numel()].view_as(w)
                for w, off in zip(ws, offs)]

    @staticmethod
    def _stack_views(group, mirror, pairs):
        ws = []
        for l1, l2 in pairs:
            ia = next(i for i, q in enumerate(group.params)
                      if q is l1.weight)
            off = group.offsets[ia]
            n = l1.weight.numel()
            ws.append(mirror[off:off + 2 * n].view(2, *l1.weight.shape))
        return ws

    @torch.no_grad()
    def refresh_bf16(self, which: str = "all") -> None:
        if not self._bf16:
            return
        if which in ("all", "critic"):
            self._critic_bf16.copy_(self.critic_group.flat_data)
        if which in ("all", "target"):
            self._target_bf16.copy_(self.target_group.flat_data)
        if which in ("all", "actor"):
            self._actor_bf16.copy_(self.actor_group.flat_data)

    def attach_ddp(self, ddp) -> None:
        """Join a data-parallel group: sync replicas, then every update
        all-reduces the flat gradient buffers (one RCCL message each)."""
        self.ddp = ddp
        if ddp is not None and ddp.enabled:
            ddp.broadcast_params(self.actor_group.flat_data)
            ddp.broadcast_params(self.critic_group.flat_data)
            ddp.broadcast_params(self.alpha_group.flat_data)
            self.hard_copy_targets()
            self.refresh_bf16()

    @torch.no_grad()
    def publish_params(self) -> torch.Tensor:
        """Flat weight vector for the rollout-side snapshot (matches
        workers.player.policy_params order)."""
        return self.actor_group.flat_data

    @torch.no_grad()
    def hard_copy_targets(self) -> None:
        """targets <- critics (reference soft_update tau=1.0 at run start)."""
        flat_polyak_(self.target_group, self.critic_group, 1.0)
        self.refresh_bf16("target")

    def zero_grad(self) -> None:
        self.actor_group.zero_grad()
        self.critic_group.zero_grad()
        self.alpha_group.zero_grad()
        # autograd may have detached .grad views (e.g. after state_dict load)
        self.actor_group.rebind_grads()
        self.critic_group.rebind_grads()
        self.alpha_group.rebind_grads()

    # ------------------------------------------------------------------
    def _use_fused(self, t: torch.Tensor) -> bool:
        from ..ops import has_native, native_enabled
        return t.is_cuda and native_enabled() and has_native()

    def _critic_q(self, states, actions):
        if self._use_fused(states):
            x = torch.cat([states, actions], dim=-1)
            if self._bf16:
                return Fops.twin_mlp_forward_bf16(x, *self._twin_local,
                                                  self._twin_local_bf16)
            return Fops.twin_mlp_forward(x, *self._twin_local)
        if self.variant in ("sac", "vsac"):
            return (self.local_critic_1(states, actions),
                    self.local_critic_2(states, actions))
        return self.local_critic(states, actions)

    def _target_q(self, states, actions):
        if self._use_fused(states):
            x = torch.cat([states, actions], dim=-1)
            if self._bf16:
                return Fops.twin_mlp_forward_bf16(x, *self._twin_target,
                                                  self._target_chain.ws16)
            return Fops.twin_mlp_forward(x, *self._twin_target)
        if self.variant in ("sac", "vsac"):
            return (self.target_critic_1(states, actions),
                    self.target_critic_2(states, actions))
        return self.target_critic(states, actions)

    def _per_sample_alpha(self, mtobss: torch.Tensor) -> torch.Tensor:
        """mtsac: per-sample alpha via one-hot gather; sac/vsac: scalar."""
        if self.variant == "mtsac":
            one_hots = mtobss[:, -self.num_tasks:]
            return Fops.gather_log_alpha(one_hots, self.log_alpha).exp().detach()
        return self.log_alpha.exp().detach()

    # -- prioritized replay ----------------------------------------------
    def _per_unsupported(self) -> None:
        """Raise for the combinations prioritized replay does not cover."""
        why = None
        if self.variant == "care":
            why = "CAREEngine has no prioritized-replay path"
        elif self.ddp is not None and getattr(self.ddp, "enabled", True):
            why = "not supported with a data-parallel group attached"
        elif self.degenerate_w and self.use_weighted_loss:
            why = "not defined for weighted_loss_mode='reference'"
        elif self.device.type == "cuda" and self._use_fused(
                self.log_alpha) and not (
                self._bf16
                and os.environ.get("DSAC_NO_MANUAL", "0") != "1"):
            why = ("on a GPU only the bf16 manual-backward path carries "
                   "importance-sampling weights (not the fp32 fused path)")
        if why is not None:
            raise NotImplementedError(f"prioritized replay: {why}")

    def attach_per(self, replay) -> None:
        """Pair with a ``sampling="prioritized"`` replay: its per_alpha /
        per_eps shape the new priorities, and every update of a batch that
        carries ``is_weights`` writes them back with
        ``replay.update_priorities`` (inside the graph when captured)."""
        self._per_unsupported()
        self._per = replay

    def _per_params(self):
        src = self._per if self._per is not None else self.cfg
        return float(src.per_alpha), float(src.per_eps)

    def per_write_back(self, replay) -> None:
        """Feed the last prioritized update's new priorities to
        ``replay``."""
        replay.update_priorities(self.per_indices, self.per_new_priorities,
                                 _zeroed=self._per_zeroed)
        self._per_zeroed = False

    def _critic_loss_per(self, states, actions, y, isn):
        """Eager critic losses with normalised IS weights ``isn [B, 1]``
        on the per-row squared errors (and on the task weights, if on);
        also returns the two TD errors."""
        if self.variant in ("sac", "vsac"):
            q1 = self.local_critic_1(states, actions)
            q2 = self.local_critic_2(states, actions)
        else:
            q1, q2 = self.local_critic(states, actions)
        d1, d2 = y - q1, y - q2
        wi = isn
        if self.use_weighted_loss:
            w = Fops.task_weights(states[:, -self.num_tasks:],
                                  self.log_alpha.exp().detach())
            wi = w.unsqueeze(-1) * isn
        q_loss = (wi * d1 ** 2).mean() + (wi * d2 ** 2).mean()
        return q_loss, d1.detach(), d2.detach()

    def update(self, batch: Dict[str, torch.Tensor]) -> Dict[str, float]:
        """One SAC gradient update; returns scalar metrics (syncs)."""
        out = self.update_tensors(batch)
        self.update_iteration += 1
        return {k: float(v.detach()) for k, v in out.items()}

    def update_tensors(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """One SAC gradient update, returning tensor metrics (no host sync
        — hipGraph-capturable).

        Order (identical to reference update/update_SAC): TD target →
        critic step → actor step → alpha step → Polyak.

        A batch from a prioritized replay (keys ``is_weights``,
        ``indices``) weights the critic loss with ``w / max w`` and leaves
        the rows' new priorities in ``per_new_priorities``; with a replay
        attached (:meth:`attach_per`) they are written back here.
        """
        per = "is_weights" in batch
        if per:
            self._per_unsupported()
        out = self._update_tensors(batch)
        if per and self._per is not None:
            self.per_write_back(self._per)
        return out

    def _update_tensors(self, batch):
        if self._use_fused(batch["states"]):
            if self.degenerate_w and self.use_weighted_loss:
                raise RuntimeError(
                    "weighted_loss_mode='reference' (degenerate broadcast) "
                    "is a CPU strict-parity mode; the fused HIP kernels "
                    "implement corrected weighting (docs/PARITY.md)")
            return self._update_tensors_fused(batch)
        states = batch["states"]
        actions = batch["actions"]
        rewards = batch["rewards"]
        next_states = batch["next_states"]
        dones = batch["dones"]

        alpha = self._per_sample_alpha(states)
        self.zero_grad()

        # --- TD target (no grad) -------------------------------------
        with torch.no_grad():
            next_actions, next_log_probs, _ = self._sample(next_states)
            q1_t, q2_t = self._target_q(next_states, next_actions)
            y = Fops.td_target(rewards, dones, q1_t, q2_t, next_log_probs,
                               alpha, self.gamma, self.reward_scale)

        # --- critic step ---------------------------------------------
        if "is_weights" in batch:
            from ..ops import torch_ref
            w = batch["is_weights"].reshape(-1, 1)
            q_loss, d1, d2 = self._critic_loss_per(states, actions, y,
                                                   w / w.max())
            self.per_indices = batch["indices"]
            self.per_new_priorities = torch_ref.per_new_priorities(
                d1, d2, *self._per_params())
            self._per_zeroed = False
        elif self.variant in ("sac", "vsac"):
            q_loss = (self.local_critic_1.cal_loss(states, actions, y)
                      + self.local_critic_2.cal_loss(states, actions, y))
        else:
            l1, l2 = self.local_critic.cal_loss(
                states, actions, y,
                use_weighted_loss=self.use_weighted_loss,
                alphas=self.log_alpha.exp().detach(),
                degenerate=self.degenerate_w)
            q_loss = l1 + l2
        q_loss.backward()
        if self.ddp is not None:
            self.ddp.allreduce_grad_(self.critic_group.flat_grad)
        self.critic_optimizer.step()

        # --- actor step ----------------------------------------------
        sampled_actions, log_probs, log_stds = self._sample(states)
        q1, q2 = self._critic_q(states, sampled_actions)
        q_min = torch.min(q1, q2)
        if self.variant == "mtsac":
            policy_loss = self.actor.cal_loss(
                log_probs, q_min, alpha,
                use_weighted_loss=self.use_weighted_loss, mtobss=states,
                alphas=self.log_alpha.exp().detach(),
                degenerate=self.degenerate_w)
        else:
            policy_loss = self.actor.cal_loss(log_probs, q_min, alpha)
        policy_loss.backward()
        if self.ddp is not None:
            self.ddp.allreduce_grad_(self.actor_group.flat_grad)
        self.actor_optimizer.step()

        # --- entropy diagnostic (reference learner.py:311-312) --------
        entropy = Fops.entropy_from_log_std(log_stds)

        # --- temperature step -----------------------------------------
        if self.variant == "mtsac":
            log_alpha_g = Fops.gather_log_alpha(
                states[:, -self.num_tasks:], self.log_alpha)
            loss_log_alpha = -(log_alpha_g * (log_probs.detach() + self.H_bar)).mean()
        else:
            loss_log_alpha = -(self.log_alpha * (log_probs.detach() + self.H_bar)).mean()
        loss_log_alpha.backward()
        if self.ddp is not None:
            self.ddp.allreduce_grad_(self.alpha_group.flat_grad)
        self.log_alpha_optimizer.step()
        self.alpha = self.log_alpha.exp().detach()

        # --- Polyak target update -------------------------------------
        flat_polyak_(self.target_group, self.critic_group, self.tau)

        return self._clip_metrics({
            "critic_loss": q_loss.detach(),
            "actor_loss": policy_loss.detach(),
            "alpha_loss": loss_log_alpha.detach(),
            "entropy": entropy.detach(),
        })

    def _actor_weights(self):
        if self.variant in ("sac", "vsac"):
            ws = [m.weight for m in self.actor.layer_intermediate] \
                + [self.actor.mu_log_std_layer.weight]
            bs = [m.bias for m in self.actor.layer_intermediate] \
                + [self.actor.mu_log_std_layer.bias]
            return ws, bs
        lins = [m for m in self.actor.mu_log_std_layer
                if isinstance(m, nn.Linear)]
        return [m.weight for m in lins], [m.bias for m in lins]

    def _dw_arena(self, name: str, numel: int, B: int):
        """[S, group_numel] fp32 split-K arena for one backward phase:
        every layer's partials land at its flat-gradient offsets, and ONE
        k_reduce_arena launch folds the whole phase's gradient (instead of
        one reduce per layer).  chunk targets ~8 batch splits, rounded to
        the 64-row GEMM tile."""
        store = self._dw_arenas
        key = (name, numel, B)
        if key not in store:
            if name.endswith("@rowblocks"):
                # one arena row per 64-row block (fused narrow backward)
                S = (B + 63) // 64
                chunk = 64
            else:
                chunk = ((B + 7) // 8 + 63) // 64 * 64
                S = (B + chunk - 1) // chunk
            store[key] = (torch.empty(S, numel, device=self.device),
                          S, chunk)
        return store[key]

    @torch.no_grad()
    def _update_tensors_manual(self, batch):
        """bf16 path with HAND-ROLLED backward: every gradient-producing
        kernel writes straight into the flat fp32 gradient buffers (no
        autograd bookkeeping, no AccumulateGrad adds, no zero_grad except
        the tiny atomically-accumulated alpha grad).  Numerically identical
        to the autograd bf16 path (same kernels, same order) — verified by
        the manual-vs-autograd GPU test.

        Structured as three SEGMENTS split at the two DP all-reduce
        boundaries so the data-parallel path can hipGraph-capture each
        segment and run the (non-capturable) RCCL collectives eagerly
        between replays — see :meth:`capture_dp`:
          seg1: forwards + TD target + critic backward  -> critic grad
          seg2: critic Adam + actor/alpha forwards+backwards -> aa grads
          seg3: actor+alpha fused Adam + target update
        Both engines run this sequence.  The segments hand their state on
        in the plain dict ``_dp_st``; each sets every key the next reads.
        :class:`CAREEngine` has its own seg1 and seg2 head (encoders) and
        shares the steps: :meth:`_squash_cat`, :meth:`_critic_loss_step`,
        :meth:`_actor_alpha_backward`, seg3 with :meth:`_update_targets`.
        """
        self._manual_seg1(batch)
        self._allreduce_critic_grads()
        self._manual_seg2()
        if self.ddp is not None:
            self.ddp.allreduce_grad_(self._aa_arena)
        return self._manual_seg3()

    def _allreduce_critic_grads(self) -> None:
        """The collectives due between the critic backward and its Adam."""
        if self.ddp is not None:
            self.ddp.allreduce_grad_(self.critic_group.flat_grad)

    @property
    def _use_krng(self) -> bool:
        """Counter-based device RNG inside the squash / replay-sample
        kernels (round 2): replaces the torch rand+randn launches and the
        hipGraph RNG-offset bookkeeping kernels.  DSAC_KRNG=0 restores
        torch's philox draws."""
        return (self._bf16
                and self._rng_ctr is not None
                and os.environ.get("DSAC_KRNG", "1") == "1")

    @property
    def _fuse_tail(self) -> bool:
        """Fused small-kernel tail of the manual update: TD target + critic
        loss fwd + bwd in one launch, actor/alpha loss fwd + bwd in one,
        the split-K arena fold inside the Adam kernels (single-GPU only:
        with DP the all-reduce sits between fold and Adam), and Polyak
        inside the actor+alpha Adam launch.  Bit-identical results;
        DSAC_FUSE_TAIL=0 restores the separate launches."""
        return os.environ.get("DSAC_FUSE_TAIL", "1") == "1"

    def _adam_prolog_all(self) -> bool:
        """ONE launch advances every optimizer's Adam state (+ RNG bump)
        at the top of seg2; the individual steppers then skip their own
        prolog launches.  Returns False (fall back to per-step prologs)
        if any optimizer lacks device state or betas differ."""
        from ..ops import native
        opts = [self.critic_optimizer, self.actor_optimizer,
                self.log_alpha_optimizer]
        ctx = self.context_encoder_optimizer
        if ctx is not None:
            opts.append(ctx)
        if any(o._dev_state is None for o in opts):
            return False
        b1, b2 = opts[0].betas
        if any(o.betas != (b1, b2) or o.eps != opts[0].eps for o in opts):
            return False
        native().adam_prolog_many(
            [o._dev_state for o in opts], [o.lr for o in opts], b1, b2,
            self._rng_ctr if self._use_krng else None)
        return True

    @torch.no_grad()
    def _manual_seg1(self, batch):
        """Segment 1: batched actor forward + squash, TD target, critic
        loss forward + backward.  Ends with the critic flat gradient ready
        for all-reduce."""
        from ..ops import native
        ext = native()
        states, next_states = batch["states"], batch["next_states"]
        B = states.shape[0]
        # ONE launch re-packs every pre-step weight set into the
        # fragment layout (critic fwd+dx, target fwd, actor fwd+dx)
        pack_chains(ext, [(self._critic_chain, True, True),
                          (self._target_chain, True, False),
                          (self._actor_chain, True, True)])

        # ---- batched actor forward + squash --------------------------
        out, acts_a = self._actor_chain.forward(next_states, states,
                                                rowcat=True)
        a_cat, lp_cat, tanh_u, ls_cat, lsr, eps = self._squash_cat(out, B)

        # ---- TD-target twin + critic twin: independent chains of one
        # shape, ONE launch (each alone fills 160 of 256 CUs) ------------
        ((q1_t, q2_t), _), ((q1, q2), acts_c) = forward_pair(
            (self._target_chain, (next_states, a_cat[:B]),
             {"save_acts": False}),
            (self._critic_chain, (states, batch["actions"]), {}))
        closs, dy = self._critic_loss_step(batch, q1_t, q2_t, lp_cat[:B],
                                           q1, q2)
        arena_c, S_c, ch_c = self._dw_arena("critic",
                                            self.critic_group.numel, B)
        self._critic_chain.backward(dy, acts_c, arena_c, S_c, ch_c)
        # single-GPU: the critic Adam kernel folds the arena itself; with
        # DP the all-reduce needs the folded gradient first
        fold_c = self._fuse_tail and self.ddp is None
        if not fold_c:
            ext.reduce_arena(arena_c, self.critic_group.flat_grad, S_c)
        self._dp_st = {
            "arena_c": (arena_c, S_c) if fold_c else None,
            "states": states, "sa": a_cat[B:], "lp": lp_cat[B:],
            "lsr": lsr, "ls_cat": ls_cat, "eps": eps, "tanh_u": tanh_u,
            "acts_a": acts_a, "closs": closs, "B": B,
        }

    def _squash_cat(self, out: torch.Tensor, B: int):
        """Squash the batched [next | current] actor output ``[2B, 2A]``
        (mu | raw log-std, read in place).  Returns ``a_cat, lp_cat,
        tanh_u, ls_cat, lsr, eps``: rows ``[:B]`` feed the TD target, rows
        ``[B:]`` the actor step and its backward."""
        from ..ops import native
        A = out.shape[1] // 2
        mu, lsr = out[:, :A], out[:, A:]
        # eps GENERATED inside the squash kernel (counter RNG) and written
        # out for the backward — no randn launch
        krng = self._use_krng and not self._eps_queue
        eps = self._eps_cat(mu, B, in_kernel=krng)
        a_cat, lp_cat, tanh_u, ls_cat = native().squashed_gaussian_fwd(
            mu, lsr, eps, float(self.actor.k),
            self._rng_ctr if krng else None)
        return a_cat, lp_cat, tanh_u, ls_cat, lsr, eps

    def _critic_loss_step(self, batch, q1_t, q2_t, nlp, q1, q2):
        """TD target + critic loss forward + backward on the four twin
        heads.  Returns ``closs`` (the loss kernel's metric slots) and
        ``dy``, the bf16 gradient at the critic heads."""
        from ..ops import native
        ext = native()
        states, rewards, dones = (batch["states"], batch["rewards"],
                                  batch["dones"])
        T = self.num_tasks
        use_w = self.use_weighted_loss
        la_det = self.log_alpha.detach()
        # one launch for TD target + loss fwd + dq (its grid covers the
        # batch in <= 32 blocks); a larger batch keeps the three launches
        fuse_loss = self._fuse_tail and states.shape[0] <= 8192
        if not fuse_loss:
            y = ext.td_target_mt(rewards, dones, q1_t, q2_t, nlp, states,
                                 la_det, T, self.gamma, self.reward_scale)
        if "is_weights" in batch:
            if not fuse_loss:
                raise NotImplementedError(
                    "prioritized replay: the IS-weighted critic loss is "
                    "the fused kernel only (B <= 8192, DSAC_FUSE_TAIL=1)")
            # with a replay attached the kernel also zeroes the sampled
            # leaves, the first step of the write-back that follows
            prio = self._per.per_prio if self._per is not None else None
            closs, dy, newp = ext.critic_td_loss_per(
                rewards, dones, q1_t, q2_t, nlp, q1, q2, states, la_det, T,
                int(use_w), self.gamma, self.reward_scale, self._loss_ws,
                batch["is_weights"], *self._per_params(), prio,
                batch["indices"] if prio is not None else None)
            self.per_indices = batch["indices"]
            self.per_new_priorities = newp
            self._per_zeroed = prio is not None
        elif fuse_loss:
            closs, dy = ext.critic_td_loss(
                rewards, dones, q1_t, q2_t, nlp, q1, q2, states, la_det, T,
                int(use_w), self.gamma, self.reward_scale, self._loss_ws)
        else:
            closs = ext.critic_loss_fwd(q1, q2, y, states, la_det, T,
                                        int(use_w), self._loss_ws)[0]
            dy = ext.critic_loss_bwd2(q1, q2, y, states, la_det, closs, T,
                                      int(use_w))
        return closs, dy

    @torch.no_grad()
    def _manual_seg2(self):
        """Segment 2: critic Adam (mirror refreshed in-kernel), actor-side
        twin forward on the post-step critic, actor/alpha losses and full
        manual backward.  Ends with the fused actor+alpha gradient arena
        ready for all-reduce."""
        from ..ops import native
        st = self._dp_st
        st["prolog"] = self._adam_prolog_all()
        # adam kernel also refreshes the bf16 mirror
        self.critic_optimizer.step(pre_prologed=st["prolog"],
                                   arena=st["arena_c"])
        # re-pack the POST-Adam critic (fwd + dx) in one launch
        pack_chains(native(), [(self._critic_chain, True, True)])
        states = st["states"]
        (aq1, aq2), acts_f = self._critic_chain.forward(states, st["sa"])
        self._actor_alpha_backward(aq1, aq2, acts_f, states.shape[1])

    def _actor_alpha_backward(self, aq1, aq2, acts_f, lo: int) -> None:
        """Seg2 from the loss kernels on: actor/alpha losses on the
        post-step twin ``aq1, aq2``, dQ/d(action) back through the critic
        chain (``lo``: width of its first input, which takes no gradient),
        squash backward, actor chain backward on the current-state rows.
        Leaves ``st["al"]`` (metric slots) and ``st["arena_a"]`` (the
        actor split-K arena for seg3 to fold, or None once folded)."""
        from ..ops import native
        ext = native()
        st = self._dp_st
        states, lp, B = st["states"], st["lp"], st["B"]
        T = self.num_tasks
        use_w = self.use_weighted_loss
        la_det = self.log_alpha.detach()
        ls = st["ls_cat"][B:]
        fuse = self._fuse_tail
        # the fwd kernel zeroes the alpha flat grad in passing (the bwd's
        # atomics target) — no separate fill launch
        if fuse and B <= 8192:
            # forward metrics, dq/dlp and the alpha flat grad in one launch.
            # The weighted-loss normalizer is the one the critic loss of
            # this update finalized (closs[2]: same states, same log_alpha
            # — alpha steps in seg3), so the blocks need not recompute it.
            al, daq, dlp = ext.actor_alpha_loss_fwd_bwd(
                aq1, aq2, lp, ls, states, la_det,
                self.alpha_group.flat_grad, T, int(use_w), self.H_bar_f,
                self._aafb_ws, st["closs"][2:3] if use_w else None)
        else:
            al = ext.actor_alpha_loss_fwd(aq1, aq2, lp, ls, states,
                                          la_det, T, int(use_w),
                                          self.H_bar_f,
                                          self.alpha_group.flat_grad,
                                          self._aloss_ws)
            daq, dlp = ext.actor_alpha_loss_bwd2(
                aq1, aq2, lp, states, la_det, al,
                self.alpha_group.flat_grad, T, int(use_w), self.H_bar_f,
                self._dla_ws)
        # dQ/d(action) only ([2, B, A] fp32 on the chain kernels); the twin
        # heads are summed inside squash bwd2
        dsa = self._critic_chain.input_grad(daq, acts_f, lo)
        dhead = ext.squashed_gaussian_bwd2(
            dsa, dlp, st["lsr"][B:], st["ls_cat"][B:], st["eps"][B:],
            st["tanh_u"][B:], float(self.actor.k))
        fg_a = self.actor_group.flat_grad
        arena_a, S_a, ch_a = self._dw_arena("actor",
                                            self.actor_group.numel, B)
        self._actor_chain.backward(dhead, st["acts_a"], arena_a, S_a, ch_a,
                                   rows=slice(B, None))
        fold_a = fuse and self.ddp is None
        if not fold_a:
            ext.reduce_arena(arena_a, fg_a, S_a)
        st["arena_a"] = (arena_a, S_a) if fold_a else None
        st["al"] = al

    @torch.no_grad()
    def _manual_seg3(self):
        """Segment 3: fused actor+alpha Adam, then the target side
        (:meth:`_update_targets`)."""
        st = self._dp_st
        # fused tail: the same launch folds the actor split-K arena and
        # does the Polyak update (it reads the critic stepped in seg2)
        FusedAdam.step_many(
            [self.actor_optimizer, self.log_alpha_optimizer],
            rng_bump=(None if st["prolog"]
                      else (self._rng_ctr if self._use_krng else None)),
            pre_prologed=st["prolog"], arena0=st["arena_a"],
            polyak=self._polyak_args() if self._fuse_tail else None)
        # NOTE: self.alpha is refreshed lazily (checkpoint/_per_sample_alpha
        # recompute from log_alpha) — an exp() here would replay as a
        # ~5 µs kernel every captured step just for bookkeeping
        self._update_targets()
        closs, al = st["closs"], st["al"]
        return self._clip_metrics({
            "critic_loss": closs[6],  # summed in-kernel
            "actor_loss": al[0],
            "alpha_loss": al[2],
            "entropy": al[3],
        })

    def _polyak_args(self):
        return (self.target_group, self.critic_group, self.tau,
                self._target_bf16)

    def _update_targets(self) -> None:
        """What seg3 does after the actor+alpha Adam: the Polyak update,
        unless the fused tail did it inside that launch."""
        if not self._fuse_tail:
            flat_polyak_(*self._polyak_args())

    def _update_tensors_fused(self, batch):
        """GPU path: same math/order as update_tensors, restructured for
        the hardware (numerically identical):

        - ONE actor forward + squash over cat(next_states, states) — both
          use pre-actor-step weights (reference samples current actions
          after the critic step, but actor weights are unchanged until the
          actor step); backward runs only on the grad-carrying states half;
        - target-critic TD forward overlaps the local-critic loss forward
          on a side stream (independent weight sets, both pre-critic-step);
        - fused loss kernels, grouped twin-Q GEMMs, one fused Adam launch
          for actor+alpha."""
        from ..ops import native
        states = batch["states"]
        actions = batch["actions"]
        rewards = batch["rewards"]
        next_states = batch["next_states"]
        dones = batch["dones"]
        T = self.num_tasks
        use_w = self.use_weighted_loss
        B = states.shape[0]
        A = self.cfg.action_dim

        if self._bf16 \
                and os.environ.get("DSAC_NO_MANUAL", "0") != "1":
            return self._update_tensors_manual(batch)
        self.zero_grad()

        # --- batched actor forward: [next | current] halves (both use
        # pre-actor-step weights; backward slices to the states half).
        # A side-stream overlap of the TD forward was A/B-tested and LOST
        # (cross-stream event sync in captured graphs cost ~5-25% —
        # profiles/r04_NOTES.md), so the TD block stays on the main stream.
        x_cat = torch.cat([next_states, states], dim=0)
        ws, bs = self._actor_weights()
        if self._bf16:
            out = Fops.mlp_forward_bf16(x_cat, ws, bs, self._actor_ws_bf16,
                                        grad_row_start=B)
        else:
            out = Fops.mlp_forward(x_cat, ws, bs, grad_row_start=B)
        mu, lsr = out[:, :A], out[:, A:]
        a_cat, lp_cat, ls_cat = Fops.squashed_gaussian(
            mu, lsr, self._eps_cat(mu, B), self.actor.k)
        next_actions = a_cat[:B].detach()
        next_log_probs = lp_cat[:B].detach()
        sampled_actions = a_cat[B:]
        log_probs = lp_cat[B:]
        log_stds = ls_cat[B:]

        with torch.no_grad():
            q1_t, q2_t = self._target_q(next_states, next_actions)
            y = native().td_target_mt(
                rewards, dones, q1_t, q2_t, next_log_probs, states,
                self.log_alpha.detach(), T, self.gamma, self.reward_scale)
        q1, q2 = self._critic_q(states, actions)
        l1, l2 = Fops.critic_loss(q1, q2, y, states, self.log_alpha.detach(),
                                  T, use_w)
        q_loss = l1 + l2
        q_loss.backward()
        self._allreduce_critic_grads()
        self.critic_optimizer.step()
        self.refresh_bf16("critic")

        # --- actor/alpha step (post-critic-step critic, frozen heads) --
        xa = torch.cat([states, sampled_actions], dim=-1)
        if self._bf16:
            aq1, aq2 = Fops.twin_mlp_forward_bf16(xa,
                                                  *self._twin_local_frozen,
                                                  self._twin_local_bf16)
        else:
            aq1, aq2 = Fops.twin_mlp_forward(xa, *self._twin_local_frozen)
        policy_loss, loss_log_alpha, entropy = Fops.actor_alpha_loss(
            aq1, aq2, log_probs, log_stds, states, self.log_alpha, T, use_w,
            self.H_bar_f)
        (policy_loss + loss_log_alpha).backward()
        if self.ddp is not None:
            self.ddp.allreduce_grad_(self._aa_arena)
        FusedAdam.step_many([self.actor_optimizer,
                             self.log_alpha_optimizer])
        self.alpha = self.log_alpha.exp().detach()

        flat_polyak_(self.target_group, self.critic_group, self.tau,
                     mirror=self._target_bf16)
        return self._clip_metrics({
            "critic_loss": q_loss.detach(),
            "actor_loss": policy_loss.detach(),
            "alpha_loss": loss_log_alpha.detach(),
            "entropy": entropy.detach(),
        })

    # ------------------------------------------------------------------
    # hipGraph capture: the ENTIRE update (sample gather, forward, backward,
    # three fused Adam steps, Polyak) replays as one captured graph —
    # per-step host cost collapses to one hipGraphLaunch.
    # ------------------------------------------------------------------
    def capture(self, replay, batch_size: int, warmup_iters: int = 3,
                chunk: int = 1):
        """Capture ``chunk`` FULL updates in ONE hipGraph.  hipGraphLaunch
        costs ~9 µs/node host-side (~0.22 ms for the ~25-node update), so
        at chunk=1 the host launch is nearly at parity with the 0.31 ms
        GPU time; chunking amortizes it (tools/probe_graph_k.py).  Every
        captured update is complete and distinct: the device-side RNG
        counter and Adam states advance INSIDE the graph, so update i of
        a chunk samples different replay indices and different eps.  The
        metrics dict reflects the chunk's LAST update."""
        if self._use_krng and hasattr(replay, "attach_rng"):
            replay.attach_rng(self._rng_ctr)
        assert self.device.type == "cuda", "capture needs a GPU"
        if getattr(replay, "sampling", None) == "prioritized":
            # every captured update writes its new priorities back
            self.attach_per(replay)
        self._graph_chunk = max(1, int(chunk))
        torch.cuda.synchronize(self.device)
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(warmup_iters):
                self.update_tensors(replay.sample(batch_size, graph_safe=True))
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(self._graph_chunk):
                self._graph_metrics = self.update_tensors(
                    replay.sample(batch_size, graph_safe=True))
        self._graph = graph
        return graph

    def graphed_update(self) -> Dict[str, torch.Tensor]:
        """Replay the captured chunk (tensor metrics refresh in place);
        advances ``update_iteration`` by the captured chunk size."""
        self._graph.replay()
        self.update_iteration += self._graph_chunk
        return self._graph_metrics

    # ------------------------------------------------------------------
    # Data-parallel segmented capture: RCCL collectives are NOT
    # hipGraph-capturable on this ROCm stack (tools/probe_rccl_graph.py —
    # the capture probe aborts the process via the NCCL watchdog), so a DP
    # update is captured as THREE graphs split at the all-reduce
    # boundaries; replay runs g1 -> eager AR(critic grad) -> g2 -> eager
    # AR(actor+alpha arena) -> g3.  This recovers hipGraph launch
    # efficiency for ~all compute kernels while keeping the collectives
    # eager.  All graphs share one memory pool so cross-segment
    # intermediates (activations, squash state) keep stable addresses.
    # ------------------------------------------------------------------
    def capture_dp(self, replay, batch_size: int, warmup_iters: int = 3):
        if getattr(replay, "sampling", None) == "prioritized":
            raise NotImplementedError(
                "prioritized replay: not supported under data-parallel "
                "capture")
        if self._use_krng and hasattr(replay, "attach_rng"):
            replay.attach_rng(self._rng_ctr)
        assert self.device.type == "cuda", "capture needs a GPU"
        assert self._bf16, \
            "segmented DP capture runs the bf16 manual-backward path"
        torch.cuda.synchronize(self.device)
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(warmup_iters):
                # full eager DP update (including real all-reduces: warms
                # RCCL's communicator and keeps rank launch order aligned)
                self._update_tensors_manual(
                    replay.sample(batch_size, graph_safe=True))
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        g1 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1):
            self._manual_seg1(replay.sample(batch_size, graph_safe=True))
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, pool=g1.pool()):
            self._manual_seg2()
        g3 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g3, pool=g1.pool()):
            self._dp_graph_metrics = self._manual_seg3()
        self._dp_graphs = (g1, g2, g3)
        return self._dp_graphs

    def dp_graphed_update(self) -> Dict[str, torch.Tensor]:
        """Replay the segmented DP update with eager RCCL between."""
        g1, g2, g3 = self._dp_graphs
        g1.replay()
        self._allreduce_critic_grads()
        g2.replay()
        if self.ddp is not None:
            self.ddp.allreduce_grad_(self._aa_arena)
        g3.replay()
        self.update_iteration += 1
        return self._dp_graph_metrics

    # ------------------------------------------------------------------
    # Checkpointing — reference .tar schema (learner.save_checkpoint).
    # ------------------------------------------------------------------
    def checkpoint_state(self) -> Dict:
        def cpu_sd(m):
            return {k: v.cpu() for k, v in m.state_dict().items()}

        state = {
            "update_iteration": self.update_iteration,
            "total_step": self.total_step,
            "actor": cpu_sd(self.actor),
            "actor_optimizer": self.actor_optimizer.state_dict(),
            "critic_optimizer": self.critic_optimizer.state_dict(),
            "log_alpha": self.log_alpha.detach().cpu(),
            "log_alpha_optimizer": self.log_alpha_optimizer.state_dict(),
            "alpha": self.log_alpha.detach().exp().cpu(),
        }
        if self.variant in ("sac", "vsac"):
            # LunarLander…/src/learner.py:144-163 key layout (LL names the
            # counter 'episode_idx'; keep both for exact-schema readers)
            state["episode_idx"] = self.update_iteration
            state.update({
                "local_critic_1": cpu_sd(self.local_critic_1),
                "local_critic_2": cpu_sd(self.local_critic_2),
                "target_critic_1": cpu_sd(self.target_critic_1),
                "target_critic_2": cpu_sd(self.target_critic_2),
            })
        else:
            # MT10_Distributed_MTSAC/src/learner.py:157-174 key layout
            state.update({
                "local_critic": cpu_sd(self.local_critic),
                "target_critic": cpu_sd(self.target_critic),
            })
        return state

    def load_checkpoint_state(self, ckpt: Dict) -> None:
        """Inverse of checkpoint_state — also fixes the reference's broken
        learner resume (it referenced a nonexistent ``actor.optimizer``,
        LunarLander…/src/learner.py:178)."""
        # LL variant saves 'episode_idx' where MT variants save
        # 'update_iteration' (LunarLander…/src/learner.py:144-163)
        self.update_iteration = int(ckpt.get("update_iteration",
                                             ckpt.get("episode_idx", 0)))
        self.total_step = int(ckpt.get("total_step", 0))
        self.actor.load_state_dict(ckpt["actor"])
        if self.variant in ("sac", "vsac"):
            self.local_critic_1.load_state_dict(ckpt["local_critic_1"])
            self.local_critic_2.load_state_dict(ckpt["local_critic_2"])
            self.target_critic_1.load_state_dict(ckpt["target_critic_1"])
            self.target_critic_2.load_state_dict(ckpt["target_critic_2"])
        else:
            self.local_critic.load_state_dict(ckpt["local_critic"])
            self.target_critic.load_state_dict(ckpt["target_critic"])
        with torch.no_grad():
            self.log_alpha.copy_(ckpt["log_alpha"].to(self.device))
        self.alpha = self.log_alpha.exp().detach()
        if "actor_optimizer" in ckpt:
            self.actor_optimizer.load_state_dict(ckpt["actor_optimizer"])
        if "critic_optimizer" in ckpt:
            self.critic_optimizer.load_state_dict(ckpt["critic_optimizer"])
        if "log_alpha_optimizer" in ckpt:
            self.log_alpha_optimizer.load_state_dict(ckpt["log_alpha_optimizer"])
        self.refresh_bf16()  # bf16 compute mirrors must track loaded masters

