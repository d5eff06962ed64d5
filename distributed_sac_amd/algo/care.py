"""CAREEngine — the CARE / CARE(M) learner update.

Implements the reference CARE learner exactly (MT10_Distributed_CARE/src/
learner.py:281-404, MT1_Distributed_CARE/src/learner.py):

- z_context computed once per update from the context encoder (:290);
- critic loss backward carries the ONLY gradients into the context encoder
  (actor uses z_context.detach(), :326-335), applied by a separate Adam
  after the SAC update (:399);
- the actor optimizes only its mu/log_std head (:143-149) and receives the
  critic's state encoder by hard copy every update (tau=1.0 tie, :402);
- detach_z_encs=True in the actor step stops gradients into the mixture
  (:326-335);
- target Q heads Polyak at tau, target state encoder at state_encoder_tau
  (:361-367; hardcoded 0.05 in MT1: MT1…/src/learner.py:311);
- CARE(M) (use_modified_care): frozen raw 768-d embeddings, projection in
  stateEncoder.mlp_context, weighted losses.

MI355X notes: the critic flat buffer is ordered [state-encoder params |
interleaved Q-head pairs], so the two Polyak taus are two fused kernels
over flat slices, the actor-SE tie is one flat copy, and the Q heads run
as grouped twin GEMMs.  In the GPU path, forward passes whose gradients
the reference computes but discards (actor-side trunk, critic-side encoder
in the actor step) run under no_grad — numerically identical updates.
"""

from __future__ import annotations

import os
from typing import Dict, Optional

import torch
import torch.nn as nn

from ..config import SACConfig
from ..models.care import CAREActor, CARECritic
from ..models.context_encoder import contextEncoder
from ..ops import functional as Fops
from ..ops.chain import (ManualChain, forward_pair, mlp_bwd_arena,
                         pack_chains)
from ..ops.flat import FlatParams, FusedAdam, polyak_flat_
from .sac import SACEngine


class CAREEngine(SACEngine):
    def __init__(self, cfg: SACConfig, device="cpu",
                 precision: Optional[str] = None,
                 max_grad_norm: Optional[float] = None):
        assert cfg.variant == "care" and cfg.encoder is not None
        super().__init__(cfg, device, precision=precision,
                         max_grad_norm=max_grad_norm)

    # ------------------------------------------------------------------
    def _build_models(self) -> None:
        cfg, dev = self.cfg, self.device
        enc_cfg = dict(cfg.encoder)
        enc_cfg.setdefault("RoBERTa_embedding_dim", 768)
        self.enc_cfg = enc_cfg
        self.use_modified_care = cfg.use_modified_care
        self.se_tau = float(enc_cfg.get("state_encoder_tau",
                                        cfg.state_encoder_tau))
        actor_cfg = {
            "state_dim": cfg.state_dim, "action_dim": cfg.action_dim,
            "action_bound": cfg.action_bound,
            "actor_hidden_dim": cfg.actor_hidden_dim,
        }
        critic_cfg = {
            "state_dim": cfg.state_dim, "action_dim": cfg.action_dim,
            "critic_hidden_dim": cfg.critic_hidden_dim,
        }
        self.context_encoder = contextEncoder(enc_cfg,
                                              self.use_modified_care).to(dev)
        self.actor = CAREActor(actor_cfg, enc_cfg, self.use_modified_care).to(dev)
        self.local_critic = CARECritic(critic_cfg, enc_cfg,
                                       self.use_modified_care).to(dev)
        self.target_critic = CARECritic(critic_cfg, enc_cfg,
                                        self.use_modified_care).to(dev)
        self.log_alpha = nn.Parameter(torch.full(
            (cfg.num_tasks,), float(cfg.log_alpha), device=dev))
        self.H_bar = torch.tensor([-float(cfg.action_dim)], device=dev)
        self.H_bar_f = -float(cfg.action_dim)
        self.alpha = self.log_alpha.exp().detach()
        # CARE uses weighted losses iff modified CARE
        # (reference learner.update_SAC use_weighted_loss=use_modified_care)
        self.use_weighted_loss = self.use_modified_care
        # strict-parity degenerate-broadcast mode (docs/PARITY.md)
        self.degenerate_w = \
            getattr(cfg, "weighted_loss_mode", "corrected") == "reference"

    def _critic_layer_pairs(self, target: bool = False):
        c = self.target_critic if target else self.local_critic
        return self._critic_linears(c)

    def _se_then_heads(self, critic: CARECritic):
        order = list(critic.state_encoder.parameters())
        self._se_numel = sum(p.numel() for p in order)
        for l1, l2 in self._critic_linears(critic):
            order += [l1.weight, l2.weight, l1.bias, l2.bias]
        return order

    def _build_optimizers(self) -> None:
        cfg = self.cfg
        self.actor_group = FlatParams(self.actor.mu_log_std_layer.parameters())
        self.actor_se_group = FlatParams(self.actor.state_encoder.parameters(),
                                         with_grad=False)
        self.critic_group = FlatParams(self._se_then_heads(self.local_critic))
        self.target_group = FlatParams(self._se_then_heads(self.target_critic),
                                       with_grad=False)
        self.alpha_group = FlatParams([self.log_alpha])
        ctx_params = [p for p in self.context_encoder.parameters()
                      if p.requires_grad]
        self.context_group = FlatParams(ctx_params) if ctx_params else None

        self.actor_optimizer = FusedAdam(self.actor_group, lr=cfg.lr_actor)
        self.critic_optimizer = FusedAdam(
            self.critic_group, lr=cfg.lr_critic,
            ref_params=list(self.local_critic.parameters()))
        self.log_alpha_optimizer = FusedAdam(self.alpha_group, lr=cfg.lr_actor)
        self.context_encoder_optimizer = (
            FusedAdam(self.context_group,
                      lr=float(self.enc_cfg.get("lr_contextEnc", cfg.lr_actor)))
            if self.context_group is not None else None)

        self._twin_local = self._build_twin_stacks(
            self.critic_group, self._critic_layer_pairs(), with_grad=True)
        self._twin_target = self._build_twin_stacks(
            self.target_group, self._critic_layer_pairs(target=True),
            with_grad=False)
        self._twin_local_frozen = ([w.detach() for w in self._twin_local[0]],
                                   [b.detach() for b in self._twin_local[1]])
        self._aa_arena = torch.zeros(
            self.actor_group.numel + self.alpha_group.numel,
            device=self.device)
        off = self.actor_group.adopt_grad_arena(self._aa_arena, 0)
        self.alpha_group.adopt_grad_arena(self._aa_arena, off)
        self._init_bf16_mirrors()
        self._init_care_bf16()
        self.hard_copy_targets()
        self.tie_actor_state_encoder()

    def attach_ddp(self, ddp) -> None:
        self.ddp = ddp
        if ddp is not None and ddp.enabled:
            for g in (self.actor_group, self.critic_group, self.alpha_group,
                      self.actor_se_group):
                ddp.broadcast_params(g.flat_data)
            if self.context_group is not None:
                ddp.broadcast_params(self.context_group.flat_data)
            self.hard_copy_targets()
            self.refresh_bf16()  # mirrors must track broadcast params

    @torch.no_grad()
    def tie_actor_state_encoder(self) -> None:
        """actor.state_encoder <- critic.state_encoder hard copy (reference
        soft_update(..., tau=1.0), learner.py:402) as one flat copy."""
        self.actor_se_group.flat_data.copy_(
            self.critic_group.flat_data[: self._se_numel])

    def zero_grad(self) -> None:
        self.actor_group.zero_grad()
        self.critic_group.zero_grad()
        self.alpha_group.zero_grad()
        if self.context_group is not None:
            self.context_group.zero_grad()
        self.actor_group.rebind_grads()
        self.critic_group.rebind_grads()
        self.alpha_group.rebind_grads()
        if self.context_group is not None:
            self.context_group.rebind_grads()

    def _polyak_targets(self, mirror=None) -> None:
        """Q heads at tau, state encoder at state_encoder_tau — two fused
        kernels over the flat slices (reference learner.py:361-367); with
        ``mirror`` the target bf16 mirror slices refresh in-kernel."""
        se = self._se_numel
        t, s = self.target_group.flat_data, self.critic_group.flat_data
        m0 = mirror[:se] if mirror is not None else None
        m1 = mirror[se:] if mirror is not None else None
        polyak_flat_(t[:se], s[:se], self.se_tau, m0)
        polyak_flat_(t[se:], s[se:], self.tau, m1)

    # ------------------------------------------------------------------
    def _sample_care(self, mtobss, z_context, detach_z_encs=False):
        mu, log_std_raw = self.actor(mtobss, z_context, detach_z_encs)
        eps = self._next_eps(mu)
        return Fops.squashed_gaussian(mu, log_std_raw, eps, self.actor.k)

    def update_tensors(self, batch: Dict[str, torch.Tensor]):
        if "is_weights" in batch:
            self._per_unsupported()
        if self._use_fused(batch["states"]):
            if self.degenerate_w and self.use_weighted_loss:
                raise RuntimeError(
                    "weighted_loss_mode='reference' is a CPU strict-parity "
                    "mode; the fused HIP kernels implement corrected "
                    "weighting (docs/PARITY.md)")
            return self._update_tensors_fused(batch)
        states, actions = batch["states"], batch["actions"]
        rewards, next_states, dones = (batch["rewards"], batch["next_states"],
                                       batch["dones"])
        T = self.num_tasks
        alpha = Fops.gather_log_alpha(states[:, -T:],
                                      self.log_alpha).exp().detach()
        self.zero_grad()

        # z_context once per update (reference :290)
        z_context = self.context_encoder(states)
        with torch.no_grad():
            na, nlp, _ = self._sample_care(next_states, z_context)
            q1_t, q2_t = self.target_critic(next_states, z_context, na)
            y = Fops.td_target(rewards, dones, q1_t, q2_t, nlp, alpha,
                               self.gamma, self.reward_scale)

        l1, l2 = self.local_critic.cal_loss(
            states, z_context, actions, y,
            use_weighted_loss=self.use_weighted_loss, num_tasks=T,
            alphas=self.log_alpha.exp().detach(),
            degenerate=self.degenerate_w)
        q_loss = l1 + l2
        q_loss.backward(retain_graph=True)
        if self.ddp is not None:
            self.ddp.allreduce_grad_(self.critic_group.flat_grad)
        self.critic_optimizer.step()

        zc_d = z_context.detach()
        sa, lp, ls = self._sample_care(states, zc_d, detach_z_encs=True)
        q1, q2 = self.local_critic(states, zc_d, sa, detach_z_encs=True)
        q_min = torch.min(q1, q2)
        policy_loss = self.actor.cal_loss(
            lp, q_min, alpha, use_weighted_loss=self.use_weighted_loss,
            mtobss=states, num_tasks=T,
            alphas=self.log_alpha.exp().detach(),
            degenerate=self.degenerate_w)
        policy_loss.backward()
        if self.ddp is not None:
            self.ddp.allreduce_grad_(self.actor_group.flat_grad)
        self.actor_optimizer.step()

        entropy = Fops.entropy_from_log_std(ls)
        log_alpha_g = Fops.gather_log_alpha(states[:, -T:], self.log_alpha)
        loss_log_alpha = -(log_alpha_g * (lp.detach() + self.H_bar)).mean()
        loss_log_alpha.backward()
        if self.ddp is not None:
            self.ddp.allreduce_grad_(self.alpha_group.flat_grad)
        self.log_alpha_optimizer.step()
        self.alpha = self.log_alpha.exp().detach()

        self._polyak_targets()
        if self.context_encoder_optimizer is not None:
            if self.ddp is not None:
                self.ddp.allreduce_grad_(self.context_group.flat_grad)
            self.context_encoder_optimizer.step()   # grads from critic bwd
        self.tie_actor_state_encoder()
        return self._clip_metrics({
            "critic_loss": q_loss.detach(),
            "actor_loss": policy_loss.detach(),
            "alpha_loss": loss_log_alpha.detach(),
            "entropy": entropy.detach()})

    # -- bf16 fast state-encoder machinery ------------------------------
    def _init_care_bf16(self) -> None:
        if not self._bf16:
            return
        self._se_fast = True
        dev = self.device

        def mlp_linears(seq):
            return [m for m in seq if isinstance(m, nn.Linear)]

        def build(critic, group, mirror):
            se = critic.state_encoder
            mix = [m for m in se.mixture_encoders.mixtureEncoders
                   if hasattr(m, "W")]
            k = mix[0].num_encoders
            info = {"k": k,
                    "mixW": [m.W for m in mix],
                    "mixB": [m.b for m in mix],
                    "mixT": [torch.empty(k, m.W.shape[2], m.W.shape[1],
                                         dtype=torch.bfloat16, device=dev)
                             for m in mix]}
            for name, seq in (("trunk", se.trunk),
                              ("mlpctx", getattr(se, "mlp_context", None))):
                if seq is None:
                    info[name] = None
                    continue
                lins = mlp_linears(seq)
                ws = [l.weight for l in lins]
                info[name] = (ws, [l.bias for l in lins],
                              self._mirror_views(group, mirror, ws))
            # fused narrow-chain eligibility: every layer <= 64 wide,
            # <= 6 layers (k_bf16_mlp_narrow constraints)
            def narrow_ok(widths, L):
                return L <= 6 and all(w <= 64 for w in widths)
            info["mix_narrow"] = narrow_ok(
                [m.W.shape[2] for m in mix], len(mix))
            info["trunk_narrow"] = narrow_ok(
                [w.shape[0] for w in info["trunk"][0]],
                len(info["trunk"][0]))
            info["ctx_narrow"] = (info["mlpctx"] is not None and narrow_ok(
                [w.shape[0] for w in info["mlpctx"][0]],
                len(info["mlpctx"][0])))
            return info

        self._se_local = build(self.local_critic, self.critic_group,
                               self._critic_bf16)
        self._se_target = build(self.target_critic, self.target_group,
                                self._target_bf16)
        self._refresh_mixT()

        # original-CARE trainable context encoder (round 2): bf16 mirror
        # so the manual path can run the context chain on the fused chain
        # kernels (fwd + dx + grouped dwdb, third arena) — in both
        # DSAC_CHAIN modes
        if self.context_group is not None:
            lins = mlp_linears(self.context_encoder.modules())
            grp = self.context_group
            ws = [l.weight for l in lins]
            bs = [l.bias for l in lins]
            self._ctx_bf16 = torch.empty(grp.numel, dtype=torch.bfloat16,
                                         device=dev)
            self._ctx_bf16.copy_(grp.flat_data)
            self.context_encoder_optimizer.bf16_mirror = self._ctx_bf16
            self._ctx_chain = ManualChain(
                self._mirror_views(grp, self._ctx_bf16, ws), bs, group=grp,
                w_params=ws, b_params=bs, always_chain=True)

    @torch.no_grad()
    def _refresh_mixT(self, which: str = "all") -> None:
        if not self._se_fast:
            return
        if which in ("all", "critic"):
            for m, W in zip(self._se_local["mixT"], self._se_local["mixW"]):
                m.copy_(W.detach().permute(0, 2, 1))
        if which in ("all", "target"):
            for m, W in zip(self._se_target["mixT"],
                            self._se_target["mixW"]):
                m.copy_(W.detach().permute(0, 2, 1))

    def refresh_bf16(self, which: str = "all") -> None:
        super().refresh_bf16(which)
        self._refresh_mixT(which)
        if which == "all" and self._ctx_chain is not None:
            self._ctx_bf16.copy_(self.context_group.flat_data)

    def _se_fwd_fast(self, info, mtobss_2d, z_context):
        """stateEncoder.forward via bf16 kernels (value-identical to the
        module path up to bf16 rounding; skips the reference's divide by
        alpha.sum(dim=1) which is exactly softmax-sum==1)."""
        # mixture encoders consume the RAW state — strip the one-hot
        # suffix (reference stateEncoder.mtobss2states_taskIndices)
        states_2d = mtobss_2d[:, : mtobss_2d.shape[1] - self.num_tasks]
        z_encs = Fops.grouped_mlp_bf16(states_2d, info["mixW"],
                                       info["mixB"], info["mixT"],
                                       info["k"])              # [k,B,50] f32
        tws, tbs, twsh = info["trunk"]
        logits = Fops.mlp_forward_bf16(z_context.detach(), tws, tbs, twsh)
        alpha = torch.softmax(logits, dim=-1)                  # [B,k]
        z_enc = (z_encs * alpha.t().unsqueeze(-1)).sum(0)      # [B,50]
        if info["mlpctx"] is not None:
            cws, cbs, cwsh = info["mlpctx"]
            zc = Fops.mlp_forward_bf16(z_context, cws, cbs, cwsh)
        else:
            zc = z_context
        return torch.cat([zc, z_enc], dim=1)

    def _twin_fwd(self, x, which: str):
        if self._bf16:
            if which == "target":
                return Fops.twin_mlp_forward_bf16(x, *self._twin_target,
                                                  self._target_chain.ws16)
            if which == "frozen":
                return Fops.twin_mlp_forward_bf16(x,
                                                  *self._twin_local_frozen,
                                                  self._twin_local_bf16)
            return Fops.twin_mlp_forward_bf16(x, *self._twin_local,
                                              self._twin_local_bf16)
        if which == "target":
            return Fops.twin_mlp_forward(x, *self._twin_target)
        if which == "frozen":
            return Fops.twin_mlp_forward(x, *self._twin_local_frozen)
        return Fops.twin_mlp_forward(x, *self._twin_local)

    def _update_tensors_fused(self, batch):
        """GPU path: fused losses + twin-head grouped GEMMs (bf16 mirrors
        when enabled).  Forwards whose grads the reference discards run
        under no_grad (see module doc); the actor head runs ONE batched
        pass over cat(next, states) like the SAC engine (the actor-side
        state encoder is no-grad in both halves)."""
        manual_ok = self._se_fast and (
            self.use_modified_care
            or self._ctx_chain is not None)
        if manual_ok and os.environ.get("DSAC_NO_MANUAL", "0") != "1":
            return self._update_tensors_manual(batch)
        from ..ops import native
        states, actions = batch["states"], batch["actions"]
        rewards, next_states, dones = (batch["rewards"], batch["next_states"],
                                       batch["dones"])
        T = self.num_tasks
        use_w = self.use_weighted_loss
        B = states.shape[0]
        A = self.actor.action_dim
        self.zero_grad()

        z_context = self.context_encoder(states)
        zc_d = z_context.detach()

        # ONE batched local-SE forward over [next | current]: the actor's
        # tied encoder equals the pre-step critic encoder (hard copy at the
        # end of every update), so its encodings are the same VALUES — the
        # states half doubles as the critic-loss encoding (with grad), and
        # a detached copy feeds the actor head.
        x_cat = torch.cat([next_states, states], dim=0)
        if self._se_fast:
            z2 = torch.cat([z_context, z_context], dim=0)
            enc_cat = self._se_fwd_fast(self._se_local, x_cat, z2)
        else:
            with torch.no_grad():
                z2 = torch.cat([zc_d, zc_d], dim=0)
                enc_cat = self.actor.state_encoder(z2, x_cat,
                                                   detach_z_encs=True)
        ws, bs = self._actor_weights()
        enc_actor_in = (enc_cat.detach() if self._se_fast
                        else enc_cat)
        if self._bf16:
            mu_lsr = Fops.mlp_forward_bf16(enc_actor_in, ws, bs,
                                           self._actor_ws_bf16,
                                           grad_row_start=B)
        else:
            mu_lsr = Fops.mlp_forward(enc_actor_in, ws, bs, grad_row_start=B)
        mu = mu_lsr[:, :A]
        lsr = mu_lsr[:, A:]
        a_cat, lp_cat, ls_cat = Fops.squashed_gaussian(
            mu, lsr, self._eps_cat(mu, B), self.actor.k)
        na, nlp = a_cat[:B].detach(), lp_cat[:B].detach()
        sa, lp, ls = a_cat[B:], lp_cat[B:], ls_cat[B:]

        with torch.no_grad():
            if self._se_fast:
                enc_t = self._se_fwd_fast(self._se_target, next_states,
                                          z_context)
            else:
                enc_t = self.target_critic.encode(next_states, z_context)
            xt = torch.cat([enc_t, na], dim=-1)
            q1_t, q2_t = self._twin_fwd(xt, "target")
            y = native().td_target_mt(rewards, dones, q1_t, q2_t, nlp,
                                      states, self.log_alpha.detach(), T,
                                      self.gamma, self.reward_scale)

        if self._se_fast:
            enc = enc_cat[B:]
        else:
            enc = self.local_critic.encode(states, z_context)
        x = torch.cat([enc, actions], dim=-1)
        q1, q2 = self._twin_fwd(x, "local")
        l1, l2 = Fops.critic_loss(q1, q2, y, states, self.log_alpha.detach(),
                                  T, use_w)
        q_loss = l1 + l2
        q_loss.backward()
        self._allreduce_critic_grads()
        self.critic_optimizer.step()
        self.refresh_bf16("critic")

        with torch.no_grad():
            if self._se_fast:
                enc_c = self._se_fwd_fast(self._se_local, states, zc_d)
            else:
                enc_c = self.local_critic.encode(states, zc_d,
                                                 detach_z_encs=True)
        xa = torch.cat([enc_c, sa], dim=-1)
        aq1, aq2 = self._twin_fwd(xa, "frozen")
        policy_loss, loss_log_alpha, entropy = Fops.actor_alpha_loss(
            aq1, aq2, lp, ls, states, self.log_alpha, T, use_w, self.H_bar_f)
        (policy_loss + loss_log_alpha).backward()
        if self.ddp is not None:
            self.ddp.allreduce_grad_(self._aa_arena)
        FusedAdam.step_many([self.actor_optimizer, self.log_alpha_optimizer])
        self.refresh_bf16("actor")
        self.alpha = self.log_alpha.exp().detach()

        self._polyak_targets()
        self.refresh_bf16("target")
        if self.context_encoder_optimizer is not None:
            self.context_encoder_optimizer.step()
        self.tie_actor_state_encoder()
        return self._clip_metrics({
            "critic_loss": q_loss.detach(),
            "actor_loss": policy_loss.detach(),
            "alpha_loss": loss_log_alpha.detach(),
            "entropy": entropy.detach()})


    # -- hand-rolled backward (modified CARE, bf16) ----------------------
    @torch.no_grad()
    def _se_fwd_manual(self, info, states_bf16, zc16, save=False, rep=1):
        """stateEncoder forward on raw kernels, optionally saving the
        activations the manual backward needs.  Value-identical to
        :meth:`_se_fwd_fast` up to bf16 rounding (the attention pool runs
        in one fused kernel, fp32 accumulate).

        ``rep=2``: the batched [next | current] call — ``zc16`` carries
        ONE copy of z_context (B rows) and the trunk / context
        projections run once on it (round-1 computed them on duplicated
        2B rows); the fused pool indexes alpha/hc by ``row % B`` and
        writes the CONCATENATED head input directly (no torch.cat)."""
        from ..ops import native
        ext = native()
        k = info["k"]
        sv = 1 if save else 0
        tws, tbs, twsh = info["trunk"]
        all_narrow = (info["mix_narrow"] and info["trunk_narrow"]
                      and (info["mlpctx"] is None or info["ctx_narrow"]))
        if all_narrow:
            # round 2: the whole SE forward's independent chains
            # (mixture G=k, trunk, mlp_context) run in ONE launch
            xs = [states_bf16, zc16]
            wss = [list(info["mixT"]), list(twsh)]
            bss = [list(info["mixB"]), [b.contiguous() for b in tbs]]
            Gs, als, ofs = [k, 1], [0, 0], [1, 1]
            if info["mlpctx"] is not None:
                cws_, cbs_, cwsh_ = info["mlpctx"]
                xs.append(zc16)
                wss.append(list(cwsh_))
                bss.append([b.contiguous() for b in cbs_])
                Gs.append(1)
                als.append(0)
                ofs.append(0)
            res = ext.mlp_narrow_fwd_multi(xs, wss, bss, Gs, als, ofs, sv)
            z_encs = res[0][0]
            acts_m = [states_bf16] + list(res[0][1:])
            h = res[1][0]
            acts_t = [zc16] + list(res[1][1:])
            if info["mlpctx"] is not None:
                hc = res[2][0]
                acts_c = [zc16] + list(res[2][1:])
                alpha, enc = ext.attn_pool_fwd_enc(h, z_encs, hc, rep)
                if save:
                    return enc, dict(acts_m=acts_m, z_encs=z_encs,
                                     acts_t=acts_t, alpha=alpha,
                                     acts_c=acts_c, rep=rep)
                return enc, None
            alpha, enc = ext.attn_pool_fwd_enc(h, z_encs, zc16, rep)
            if save:
                return enc, dict(acts_m=acts_m, z_encs=z_encs,
                                 acts_t=acts_t, alpha=alpha, acts_c=None,
                                 rep=rep)
            return enc, None
        if info["mix_narrow"]:
            res = ext.mlp_narrow_fwd_bf16(states_bf16, info["mixT"],
                                          list(info["mixB"]), k, 0, 1, sv)
            z_encs = res[0]                      # f32 [k,M,D]
            acts_m = [states_bf16] + res[1:]
        else:
            acts_m = [states_bf16]
            h = states_bf16
            nm = len(info["mixT"])
            z_encs = None
            for i in range(nm):
                last = i == nm - 1
                h = ext.linear_act_fwd_bf16(h, info["mixT"][i],
                                            info["mixB"][i],
                                            0 if last else 1, k,
                                            1 if last else 0)
                if last:
                    z_encs = h
                else:
                    acts_m.append(h)
        if info["trunk_narrow"]:
            res = ext.mlp_narrow_fwd_bf16(zc16, twsh, list(tbs), 1, 0, 1, sv)
            h = res[0]                           # logits f32
            acts_t = [zc16] + res[1:]
        else:
            acts_t = [zc16]
            h = zc16
            nt = len(twsh)
            for i in range(nt):
                last = i == nt - 1
                h = ext.linear_act_fwd_bf16(h, twsh[i], tbs[i].contiguous(),
                                            0 if last else 1, 1,
                                            1 if last else 0)
                if not last:
                    acts_t.append(h)
        if info["mlpctx"] is None:
            # original CARE: no mlp_context — enc = [z_context | z_enc]
            alpha, enc = ext.attn_pool_fwd_enc(h, z_encs, zc16, rep)
            if save:
                return enc, dict(acts_m=acts_m, z_encs=z_encs,
                                 acts_t=acts_t, alpha=alpha, acts_c=None,
                                 rep=rep)
            return enc, None
        cws, cbs, cwsh = info["mlpctx"]
        if info["ctx_narrow"]:
            res = ext.mlp_narrow_fwd_bf16(zc16, cwsh, list(cbs), 1, 0, 0, sv)
            hc = res[0]                          # zc projection, bf16
            acts_c = [zc16] + res[1:]
        else:
            acts_c = [zc16]
            hc = zc16
            nc = len(cwsh)
            for i in range(nc):
                last = i == nc - 1
                hc = ext.linear_act_fwd_bf16(hc, cwsh[i],
                                             cbs[i].contiguous(),
                                             0 if last else 1, 1, 0)
                if not last:
                    acts_c.append(hc)
        alpha, enc = ext.attn_pool_fwd_enc(h, z_encs, hc, rep)
        if save:
            return enc, dict(acts_m=acts_m, z_encs=z_encs, acts_t=acts_t,
                             alpha=alpha, acts_c=acts_c, rep=rep)
        return enc, None

    # The three-segment manual update itself is SACEngine's
    # (_update_tensors_manual, capture_dp, dp_graphed_update); CARE
    # brings its own seg1 and seg2 head and the hooks below.
    @property
    def _fuse_tail(self) -> bool:
        # CARE keeps the separate tail launches it has always had: nobody
        # has measured it on the fused tail
        return False

    def _allreduce_critic_grads(self) -> None:
        super()._allreduce_critic_grads()
        # context_group exists exactly for original CARE: the modified
        # contextEncoder is one frozen embedding, the original one always
        # has its trainable embedding header (_build_optimizers keeps
        # the requires_grad parameters)
        if self.ddp is not None and self.context_group is not None:
            self.ddp.allreduce_grad_(self.context_group.flat_grad)

    @torch.no_grad()
    def _manual_seg1(self, batch):
        """CARE's segment 1, both variants (CARE(M) frozen context,
        original CARE trainable context encoder): z_context, one batched
        state-encoder forward under the actor head, the target state
        encoder under the TD heads, and after the critic chain backward
        the state-encoder (and context) backward: critic and context
        gradients.  Reference gradient-flow rules
        (MT10_Distributed_CARE/src/learner.py:281-404): trunk input
        detached, the actor optimizes only its head, context gradients
        come from the critic loss only."""
        from ..ops import native
        ext = native()
        states, next_states = batch["states"], batch["next_states"]
        T = self.num_tasks
        B = states.shape[0]
        sd = states.shape[1] - T                 # raw state dim
        info = self._se_local
        orig = not self.use_modified_care
        # ONE launch re-packs every pre-step weight set
        pack_chains(ext, [(self._critic_chain, True, True),
                          (self._target_chain, True, False),
                          (self._actor_chain, True, True)]
                    + ([(self._ctx_chain, True, True)] if orig else []))

        if orig:
            # original CARE: TRAINABLE context encoder (embedding header +
            # mlp) — forward on the fused chain kernel over the gathered
            # frozen embeddings; activations saved for the third-arena
            # backward below (reference MT1…/learner.py: context grads
            # come from the critic loss only)
            idx = states[:, -T:].argmax(dim=1)
            emb = torch.relu(self.context_encoder.embedding[0](idx))
            z_context, acts_ctx = self._ctx_chain.forward(emb)
        else:
            z_context = self.context_encoder(states)     # frozen embedding
            acts_ctx = None
        zc_dim = (self._se_local["mlpctx"][0][-1].shape[0]
                  if self._se_local["mlpctx"] is not None
                  else z_context.shape[1])
        zc16 = z_context.to(torch.bfloat16)

        # ---- ONE batched local-SE forward over [next | current]; the
        # trunk / context projections run ONCE on the (identical) z rows
        x_cat = torch.cat([next_states[:, :sd], states[:, :sd]], dim=0)
        enc_cat, se_saved = self._se_fwd_manual(info, x_cat.to(torch.bfloat16),
                                                zc16, save=True, rep=2)

        # ---- batched actor head + squash ------------------------------
        out, acts_a = self._actor_chain.forward(enc_cat)
        a_cat, lp_cat, tanh_u, ls_cat, lsr, eps = self._squash_cat(out, B)

        # ---- TD target (target SE + target heads, no grad) ------------
        enc_t, _ = self._se_fwd_manual(self._se_target,
                                       next_states[:, :sd].to(torch.bfloat16),
                                       zc16)
        # target heads + critic heads: independent chains, ONE launch
        ((q1_t, q2_t), _), ((q1, q2), acts_q) = forward_pair(
            (self._target_chain, (enc_t, a_cat[:B]), {"save_acts": False}),
            (self._critic_chain, (enc_cat[B:], batch["actions"]), {}))

        # ---- critic loss + manual backward ----------------------------
        closs, dy = self._critic_loss_step(batch, q1_t, q2_t, lp_cat[:B],
                                           q1, q2)
        fg_c = self.critic_group.flat_grad
        arena_c, S_c, ch_c = self._dw_arena("critic",
                                            self.critic_group.numel, B)
        dx0 = self._critic_chain.backward(dy, acts_q, arena_c, S_c, ch_c,
                                          dx0_lo=0)        # bf16 [B, se+A]
        # state-encoder backward (states half of the batched acts)
        zen = se_saved["z_encs"][:, B:].contiguous()     # f32 [k,B,D]
        dedup = se_saved.get("rep", 1) == 2
        alpha_cur = (se_saved["alpha"] if dedup
                     else se_saved["alpha"][B:])
        dzencs, dlogits = ext.attn_pool_bwd(zen, alpha_cur,
                                            dx0, dx0.shape[1], zc_dim)
        mlpctx = info["mlpctx"]
        if mlpctx is not None:
            cws, cbs, cwsh = mlpctx
        tws, tbs, twsh = info["trunk"]
        acts_m = ([se_saved["acts_m"][0][B:]]
                  + [a[:, B:].contiguous() for a in se_saved["acts_m"][1:]])
        base = fg_c.data_ptr()

        def offs(ps):
            return [(p_.grad.data_ptr() - base) // 4 for p_ in ps]

        def cur_half(acts):
            return acts if dedup else [a[B:] for a in acts]
        use_fused_se_bwd = (
            os.environ.get("DSAC_NARROW_BWD", "1") == "1"
            and info["mix_narrow"] and info["trunk_narrow"]
            and (mlpctx is None or info["ctx_narrow"]))
        if use_fused_se_bwd:
            # DEFAULT ON since round 2: GPU-validated (exact parameter
            # agreement vs the per-layer arena path, +3.8% eager rate —
            # gpurun_out r2 call1 / tests/test_gpu_kernels.py narrow gate
            # test); whole-chain fused backward, one launch per chain,
            # partials per 64-row block.  DSAC_NARROW_BWD=0 restores the
            # per-layer path.
            arena2, S2, _ = self._dw_arena("se@rowblocks",
                                           self.critic_group.numel, B)
            # all three SE backward chains in ONE launch (round 2)
            dys_l, actss, wss_l = [], [], []
            w_os, b_os, Gl, trl = [], [], [], []
            if mlpctx is not None:
                dys_l.append(dx0[:, :zc_dim].contiguous())
                actss.append(cur_half(se_saved["acts_c"]))
                wss_l.append(list(cwsh))
                w_os.append(offs(cws))
                b_os.append(offs(cbs))
                Gl.append(1)
                trl.append(0)
            dys_l.append(dlogits)
            actss.append(cur_half(se_saved["acts_t"]))
            wss_l.append(list(twsh))
            w_os.append(offs(tws))
            b_os.append(offs(tbs))
            Gl.append(1)
            trl.append(0)
            dys_l.append(dzencs)
            actss.append(acts_m)
            wss_l.append(list(info["mixT"]))
            w_os.append(offs(info["mixW"]))
            b_os.append(offs(info["mixB"]))
            Gl.append(info["k"])
            trl.append(1)
            ext.mlp_narrow_bwd_multi(dys_l, actss, wss_l, arena2,
                                     w_os, b_os, Gl, trl)
            se_n = self._se_numel
            ext.reduce_arena(arena2, fg_c, S2, 0, se_n)
            ext.reduce_arena(arena_c, fg_c, S_c, se_n, -1)
        else:
            if mlpctx is not None:
                mlp_bwd_arena(ext, dx0[:, :zc_dim].contiguous(),
                              cur_half(se_saved["acts_c"]), cwsh,
                              offs(cws), offs(cbs), arena_c, S_c, ch_c)
            mlp_bwd_arena(ext, dlogits, cur_half(se_saved["acts_t"]), twsh,
                          offs(tws), offs(tbs), arena_c, S_c, ch_c)
            mlp_bwd_arena(ext, dzencs, acts_m, info["mixT"],
                          offs(info["mixW"]), offs(info["mixB"]),
                          arena_c, S_c, ch_c, G=info["k"], transpose_w=1)
            ext.reduce_arena(arena_c, fg_c, S_c)
        if orig:
            # context-encoder backward: the only z_context gradient source
            # is the critic-loss concat half of dx0 (reference
            # retain_graph rule) — fused dx chain + grouped dwdb into the
            # context arena, Adam stepped at the end of the update
            arena_x, S_x, ch_x = self._dw_arena(
                "ctx", self.context_group.numel, B)
            self._ctx_chain.backward(dx0[:, :zc_dim].contiguous(), acts_ctx,
                                     arena_x, S_x, ch_x)
            ext.reduce_arena(arena_x, self.context_group.flat_grad, S_x)
        self._dp_st = dict(
            states=states, sd=sd, zc16=zc16, sa=a_cat[B:], lp=lp_cat[B:],
            ls_cat=ls_cat, B=B, eps=eps, tanh_u=tanh_u, lsr=lsr,
            acts_a=acts_a, closs=closs)

    @torch.no_grad()
    def _manual_seg2(self):
        """CARE's head of segment 2: the actor step's critic-side encoding
        comes from the POST-step state encoder."""
        from ..ops import native
        st = self._dp_st
        st["prolog"] = self._adam_prolog_all()
        # adam kernel refreshes the flat bf16 mirror
        self.critic_optimizer.step(pre_prologed=st["prolog"])
        self._refresh_mixT("critic")   # transposed mixture views still need it
        enc_c, _ = self._se_fwd_manual(
            self._se_local, st["states"][:, :st["sd"]].to(torch.bfloat16),
            st["zc16"])
        # re-pack the POST-Adam critic (fwd + dx) in one launch
        pack_chains(native(), [(self._critic_chain, True, True)])
        (aq1, aq2), acts_f = self._critic_chain.forward(enc_c, st["sa"])
        self._actor_alpha_backward(aq1, aq2, acts_f, enc_c.shape[1])

    def _update_targets(self) -> None:
        """Two-tau Polyak, then what CARE's update ends with: the context
        Adam (its gradient came from the critic backward; it refreshes the
        context mirror, its prolog ran in seg2) and the encoder tie."""
        self._polyak_targets(mirror=self._target_bf16)
        self._refresh_mixT("target")
        if self.context_encoder_optimizer is not None:
            self.context_encoder_optimizer.step(
                pre_prologed=self._dp_st["prolog"])
        self.tie_actor_state_encoder()

    @torch.no_grad()
    def publish_params(self) -> torch.Tensor:
        """[actor.state_encoder | actor head | trainable context params] —
        the CARE rollout policy needs the tied encoder and (original CARE)
        the trained context encoder (reference C3 publishes actor +
        context_encoder state_dicts, learner.py:412-422)."""
        parts = [self.actor_se_group.flat_data, self.actor_group.flat_data]
        if self.context_group is not None:
            parts.append(self.context_group.flat_data)
        return torch.cat(parts)

    # ------------------------------------------------------------------
    def checkpoint_state(self) -> Dict:
        def cpu_sd(m):
            return {k: v.cpu() for k, v in m.state_dict().items()}
        ctx_opt = (self.context_encoder_optimizer.state_dict()
                   if self.context_encoder_optimizer is not None else
                   {"state": {}, "param_groups": []})
        # MT10_Distributed_CARE/src/learner.py:178-198 key layout
        return {
            "update_iteration": self.update_iteration,
            "total_step": self.total_step,
            "context_encoder": cpu_sd(self.context_encoder),
            "context_encoder_optimizer": ctx_opt,
            "local_critic": cpu_sd(self.local_critic),
            "critic_optimizer": self.critic_optimizer.state_dict(),
            "target_critic": cpu_sd(self.target_critic),
            "actor": cpu_sd(self.actor),
            "actor_optimizer": self.actor_optimizer.state_dict(),
            "log_alpha": self.log_alpha.detach().cpu(),
            "log_alpha_optimizer": self.log_alpha_optimizer.state_dict(),
            "alpha": self.log_alpha.detach().exp().cpu(),
        }

    def load_checkpoint_state(self, ckpt: Dict) -> None:
        self.update_iteration = int(ckpt.get("update_iteration", 0))
        self.total_step = int(ckpt.get("total_step", 0))
        self.context_encoder.load_state_dict(ckpt["context_encoder"])
        self.local_critic.load_state_dict(ckpt["local_critic"])
        self.target_critic.load_state_dict(ckpt["target_critic"])
        self.actor.load_state_dict(ckpt["actor"])
        with torch.no_grad():
            self.log_alpha.copy_(ckpt["log_alpha"].to(self.device))
        self.alpha = self.log_alpha.exp().detach()
        for name, opt in (("critic_optimizer", self.critic_optimizer),
                          ("actor_optimizer", self.actor_optimizer),
                          ("log_alpha_optimizer", self.log_alpha_optimizer)):
            if name in ckpt:
                opt.load_state_dict(ckpt[name])
        if (self.context_encoder_optimizer is not None
                and "context_encoder_optimizer" in ckpt
                and ckpt["context_encoder_optimizer"].get("param_groups")):
            self.context_encoder_optimizer.load_state_dict(
                ckpt["context_encoder_optimizer"])
        self.refresh_bf16()  # bf16 mirrors (incl. mixT) track the masters
