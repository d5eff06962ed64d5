"""Dispatching functional API for the SAC hot-path ops.

On CUDA(ROCm) tensors these route to the in-tree HIP/CDNA4 extension
(required — loud failure if missing); on CPU they compose the pure-torch
reference implementations from :mod:`.torch_ref`.

The custom autograd Functions wrap a whole fused region (an entire MLP, the
full squashed-Gaussian head) so the autograd graph has one node per region
instead of one per elementwise op — the backward chain is hand-written HIP.
"""

from __future__ import annotations

import os
from typing import List, Optional, Sequence

import torch

from . import has_native, native, native_enabled
from . import torch_ref

ACT_NONE = 0
ACT_RELU = 1


def _use_native(t: torch.Tensor) -> bool:
    return t.is_cuda and native_enabled()


# ---------------------------------------------------------------------------
# Whole-chain fp32 forward (k_f32_chain_fwd): opt-in with DSAC_F32_CHAIN=1.
# Off (the default) not one launch changes.  On, an fp32 MLP forward whose
# shapes the kernel serves is ONE launch instead of one per layer, and a
# second input x2 is column-concatenated in the kernel's loader instead of
# by a torch.cat launch.  Backward is the per-layer one unless
# DSAC_F32_CHAIN_BWD=1 (below).
# ---------------------------------------------------------------------------

def f32_chain_enabled() -> bool:
    return os.environ.get("DSAC_F32_CHAIN", "0") == "1"


def _f32_chain_ok(x1, x2, ws, bs, G: int) -> bool:
    """The flag is on and mlp_chain_fwd_f32 accepts these arguments (its
    own checks would raise otherwise): contiguous fp32 device tensors, at
    most 6 layers, every width within the kernel's cap."""
    if not f32_chain_enabled() or not 1 <= len(ws) <= 6:
        return False
    ts = [x1, *ws, *bs] + ([] if x2 is None else [x2])
    if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
               for t in ts):
        return False
    if x1.dim() != 2 or (x2 is not None and (
            x2.dim() != 2 or x2.shape[0] != x1.shape[0])):
        return False
    if not all(w.dim() == 3 or (G == 1 and w.dim() == 2) for w in ws):
        return False
    cap = native().F32_CHAIN_MAX_WIDTH
    k0 = x1.shape[1] + (0 if x2 is None else x2.shape[1])
    return x1.shape[0] >= 1 and max(k0, *(w.shape[-2] for w in ws)) <= cap


def _f32_chain_nograd(x1, x2, ws, bs, G: int):
    """A forward nobody differentiates (target twin, frozen twin): no
    activation is written to global memory."""
    return native().mlp_chain_fwd_f32(x1, x2, list(ws), list(bs), G,
                                      False)[0]


# ---------------------------------------------------------------------------
# Whole-chain fp32 backward (k_f32_chain_dx, k_f32_chain_dwdb): opt-in with
# DSAC_F32_CHAIN_BWD=1, independent of DSAC_F32_CHAIN (both forward paths
# save the same tensors).  Off (the default) not one launch changes.  On,
# the backward of an fp32 MLP of two or more layers is three launches — the
# dx walk, the grouped split-K dW/db, one arena fold — instead of up to
# five per layer.
# ---------------------------------------------------------------------------

def f32_chain_bwd_enabled() -> bool:
    return os.environ.get("DSAC_F32_CHAIN_BWD", "0") == "1"


def _f32_chain_bwd_ok(dy, acts, ws, G: int) -> bool:
    """The flag is on and the chain-backward bindings accept these
    arguments: contiguous fp32 device tensors, 2 to 6 layers (a single
    layer stays per-layer), every width within the kernel's cap."""
    if not f32_chain_bwd_enabled() or not 2 <= len(ws) <= 6:
        return False
    if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
               for t in (dy, *acts, *ws)):
        return False
    if not all(w.dim() == 3 or (G == 1 and w.dim() == 2) for w in ws):
        return False
    cap = native().F32_CHAIN_MAX_WIDTH
    return dy.shape[-2] >= 1 and max(
        ws[0].shape[-1], *(w.shape[-2] for w in ws)) <= cap


def _f32_chain_bwd_slices(ws, G: int, M: int) -> int:
    """Split-K slices of the grouped dW/db launch.  Its workgroups are one
    wave each, so aim at about two waves per SIMD (8 workgroups per CU);
    a slice is at least 4 batch rows."""
    jobs = G * sum(-(-w.shape[-2] // 64) * -(-w.shape[-1] // 64) for w in ws)
    cus = torch.cuda.get_device_properties(ws[0].device).multi_processor_count
    return max(1, min(-(-8 * cus // jobs), -(-M // 4)))


def _f32_chain_bwd(dy, acts, ws, G: int, dx0_lo: int, need_w):
    """``(dx0, dws, dbs)`` of a whole chain.  ``acts[l]`` is the input of
    layer l; ``dx0_lo < 0``: no input gradient, else its columns from
    ``dx0_lo`` on.  ``dws[l]`` / ``dbs[l]`` are views of one flat tensor
    (the dW/db arena's layout: every dW in layer order, then every db) for
    the layers ``need_w`` marks, None for the others."""
    ext = native()
    n = len(ws)
    dys, dx0 = ext.mlp_chain_bwd_dx_f32(dy, list(ws), list(acts), G, dx0_lo)
    dws: List[Optional[torch.Tensor]] = [None] * n
    dbs: List[Optional[torch.Tensor]] = [None] * n
    if any(need_w):
        S = _f32_chain_bwd_slices(ws, G, dy.shape[-2])
        arena = ext.mlp_chain_bwd_dwdb_f32([*dys, dy], list(acts), G, S)
        flat = torch.empty(arena.shape[1], dtype=dy.dtype, device=dy.device)
        ext.reduce_arena(arena, flat, S)
        off = 0
        for i, w in enumerate(ws):
            if need_w[i]:
                dws[i] = flat[off:off + w.numel()].view(w.shape)
            off += w.numel()
        for i, w in enumerate(ws):
            nb = w.numel() // w.shape[-1]
            if need_w[i]:
                dbs[i] = flat[off:off + nb].view(w.shape[:-1])
            off += nb
    return dx0, dws, dbs


# ---------------------------------------------------------------------------
# Fused fp32 MLP (Linear+bias+ReLU chain, linear output layer), G stacked
# networks per launch (grouped GEMMs; the twin critic is G=2 with weights
# [2,N,K] — views into the critic's flat parameter buffer)
# ---------------------------------------------------------------------------

class _MLPF32(torch.autograd.Function):
    """Whole-MLP fused forward/backward on HIP, for G networks at once.

    forward saves post-activation intermediates; ReLU backward masks come
    from the outputs themselves (relu(y)==0 <=> grad 0).

    Layer 0 consumes the shared x (group-stride 0); later layers run on
    per-group activations [G,B,N].  Backward mirrors this: per-group dX for
    hidden layers, group-SUMMED dX at layer 0 (both Qs consume the same x —
    reference Critic.forward computes Q1(x), Q2(x) on one cat([s,a])).
    G == 1 has no group dimension anywhere, and for it both dX modes are
    the same launch.  G > 1 returns one output per head, so autograd hands
    backward one gradient per head and backward stacks them itself.

    x2 is not None: the input is [x || x2], concatenated by the chain
    kernel's loader (which also saves the concatenation for backward) —
    the caller has checked _f32_chain_ok.
    """

    @staticmethod
    def forward(ctx, x: torch.Tensor, x2: Optional[torch.Tensor],
                n_layers: int, G: int, grad_row_start: int, *wb):
        ws = wb[:n_layers]      # each [N, K], or [G, N, K]
        bs = wb[n_layers:]      # each [N], or [G, N]
        ext = native()
        if x2 is not None or _f32_chain_ok(x, None, ws, bs, G):
            h, saved = ext.mlp_chain_fwd_f32(x, x2, list(ws), list(bs),
                                             G, True)
            acts: List[torch.Tensor] = [*saved, h]
        else:
            acts = [x]
            for i in range(n_layers):
                act = ACT_RELU if i < n_layers - 1 else ACT_NONE
                acts.append(ext.linear_act_fwd_g(acts[-1], ws[i], bs[i],
                                                 act, G))
            h = acts[-1]
        ctx.save_for_backward(*acts, *ws)
        ctx.n_layers = n_layers
        ctx.G = G
        ctx.grad_row_start = grad_row_start
        ctx.c1 = x.shape[1]
        return h if G == 1 else tuple(h[g] for g in range(G))

    @staticmethod
    def backward(ctx, *grads: torch.Tensor):
        n, G = ctx.n_layers, ctx.G
        saved = ctx.saved_tensors
        acts = saved[: n + 1]
        ws = saved[n + 1:]
        ext = native()
        # forward args: (x, x2, n_layers, G, grad_row_start, *ws, *bs)
        need_x1, need_x2 = ctx.needs_input_grad[:2]
        need_w = ctx.needs_input_grad[-2 * n:-n]
        dy = grads[0] if G == 1 else torch.stack(grads, dim=0)  # [G,B,Nout]
        # rows below grad_row_start carry no gradient by construction (the
        # batched TD-side forward): slice them out of the backward chain
        # (row slices of row-major 2-D tensors stay contiguous)
        r0 = ctx.grad_row_start
        if r0:
            acts = [a[..., r0:, :] for a in acts]
            dy = dy[..., r0:, :]
        dy = dy.contiguous()
        c1 = ctx.c1             # dx[:, :c1] is x's gradient, the rest x2's
        dx = None
        if _f32_chain_bwd_ok(dy, acts[:n], ws, G):
            # only x2 needs a gradient: the dx walk skips x's columns
            lo = 0 if need_x1 else c1 if need_x2 else -1
            dx, dws, dbs = _f32_chain_bwd(dy, acts[:n], ws, G, lo, need_w)
            c1 -= max(lo, 0)
        else:
            dws, dbs = [None] * n, [None] * n
            for i in range(n - 1, -1, -1):
                # mask==1 only for hidden layers (their saved act is
                # post-ReLU)
                act = ACT_RELU if i < n - 1 else ACT_NONE
                if need_w[i]:
                    dws[i], dbs[i] = ext.linear_bwd_dwdb_g(
                        dy, acts[i], acts[i + 1], act, G)
                if i > 0:
                    dy = ext.linear_bwd_dx_g(dy, ws[i], acts[i + 1], act,
                                             G, 0)
                elif need_x1 or need_x2:
                    dx = ext.linear_bwd_dx_g(dy, ws[0], acts[1], act, G, 1)
        return (dx[:, :c1] if need_x1 else None,
                dx[:, c1:] if need_x2 else None, None, None, None,
                *dws, *dbs)


def _mlp_f32(x, x2, ws, bs, G: int, grad_row_start: int):
    """_MLPF32 on [x || x2].  x2 reaches it only when the chain-forward
    kernel takes the call; otherwise torch.cat joins the two out here, and
    autograd's own cat-backward splits the gradient.  A chain forward
    nobody differentiates returns the stacked [G,B,Nout] (indexable like
    the Function's tuple of heads)."""
    if _f32_chain_ok(x, x2, ws, bs, G):
        if not torch.is_grad_enabled():
            return _f32_chain_nograd(x, x2, ws, bs, G)
    elif x2 is not None:
        x, x2 = torch.cat([x, x2], dim=-1), None
    return _MLPF32.apply(x, x2, len(ws), G, grad_row_start, *ws, *bs)


def mlp_forward(x: torch.Tensor,
                weights: Sequence[torch.Tensor],
                biases: Sequence[torch.Tensor],
                grad_row_start: int = 0,
                x2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ReLU-hidden MLP with linear output (reference build_mlp semantics).

    grad_row_start>0: rows [0, start) are forward-only (their output grads
    are structurally zero — e.g. the TD half of a batched actor pass), so
    backward runs on the remaining rows only.

    x2: the MLP's input is [x || x2] (columns)."""
    if _use_native(x):
        return _mlp_f32(x, x2, weights, biases, 1, grad_row_start)
    if x2 is not None:
        x = torch.cat([x, x2], dim=-1)
    return torch_ref.mlp_forward(x, weights, biases)


def ln_mlp_forward(x: torch.Tensor, weights, biases, gammas, betas,
                   eps: float = torch_ref.LN_EPS) -> torch.Tensor:
    """LayerNorm MLP (hidden layers Linear -> LayerNorm -> ReLU, linear
    output).  The autograd path is the torch one, for CPU tensors; on a GPU
    the LN chain kernels are driven by ops.chain.ManualChain (the manual
    bf16 update), and nothing stands in for them here."""
    if _use_native(x):
        raise NotImplementedError(
            "critic_layer_norm: no autograd GPU path, the LN chain kernels "
            "run in the manual bf16 update only")
    return torch_ref.ln_mlp_forward(x, list(weights), list(biases),
                                    list(gammas), list(betas), eps)


def twin_mlp_forward(x: torch.Tensor, stacked_ws, stacked_bs,
                     x2: Optional[torch.Tensor] = None):
    """Both Q heads in one grouped launch per layer.  stacked_ws[i] is a
    [2,N,K] view into the critic flat parameter buffer.  x2: the input is
    [x || x2] (columns)."""
    q = _mlp_f32(x, x2, stacked_ws, stacked_bs, 2, 0)
    return q[0], q[1]


# ---------------------------------------------------------------------------
# Fused tanh-squashed Gaussian sample + log-prob
# ---------------------------------------------------------------------------

class _SquashedGaussian(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, log_std_raw, eps, k: float):
        ext = native()
        action, log_prob, tanh_u, log_std = ext.squashed_gaussian_fwd(
            mu, log_std_raw, eps, float(k))
        ctx.save_for_backward(log_std_raw, log_std, eps, tanh_u)
        ctx.k = float(k)
        ctx.mark_non_differentiable(log_std)
        return action, log_prob, log_std

    @staticmethod
    def backward(ctx, grad_action, grad_log_prob, _grad_log_std):
        log_std_raw, log_std, eps, tanh_u = ctx.saved_tensors
        ext = native()
        dmu, dlog_std_raw = ext.squashed_gaussian_bwd(
            grad_action.contiguous(), grad_log_prob.contiguous(),
            log_std_raw, log_std, eps, tanh_u, ctx.k)
        return dmu, dlog_std_raw, None, None


def squashed_gaussian(mu: torch.Tensor, log_std_raw: torch.Tensor,
                      eps: torch.Tensor, k: float):
    """Returns (action, log_prob[B,1], clamped log_std).

    Gradients flow to mu and log_std_raw (pre-clamp), reproducing the
    reference's clamp-then-rsample autograd semantics
    (LunarLander…/src/model.py:45-59).
    """
    if _use_native(mu):
        return _SquashedGaussian.apply(mu, log_std_raw, eps, k)
    return torch_ref.squashed_gaussian(mu, log_std_raw, eps, k)


# ---------------------------------------------------------------------------
# Fused SAC loss heads (reference math in kernel K6; one graph node per loss
# instead of ~15 torch glue kernels each).
# ---------------------------------------------------------------------------

class _CriticLoss(torch.autograd.Function):
    """(loss1, loss2) = (optionally task-weighted) MSE vs TD target.

    Matches reference Critic.cal_loss (MT10…MTSAC/src/model.py:157-196):
    w_i = softmax(-exp(log_alpha))[t_i] renormalized; loss = mean(w*l).
    """

    @staticmethod
    def forward(ctx, q1, q2, y, states, log_alpha_det, num_tasks: int,
                use_weighted: bool):
        ext = native()
        out = ext.critic_loss_fwd(q1.contiguous(), q2.contiguous(),
                                  y.contiguous(), states.contiguous(),
                                  log_alpha_det, num_tasks,
                                  int(use_weighted))[0]
        ctx.save_for_backward(q1, q2, y, states, log_alpha_det, out)
        ctx.meta = (num_tasks, use_weighted)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g1, g2):
        q1, q2, y, states, la, saved = ctx.saved_tensors
        T, use_w = ctx.meta
        gscale = torch.stack([g1.reshape(()), g2.reshape(())]).contiguous()
        dq1, dq2 = native().critic_loss_bwd(
            q1.contiguous(), q2.contiguous(), y.contiguous(),
            states.contiguous(), la, saved, gscale, T, int(use_w))
        return dq1, dq2, None, None, None, None, None


def critic_loss(q1, q2, y, states, log_alpha_det, num_tasks, use_weighted):
    if _use_native(q1):
        return _CriticLoss.apply(q1, q2, y, states, log_alpha_det,
                                 num_tasks, use_weighted)
    l1 = (y - q1) ** 2
    l2 = (y - q2) ** 2
    if use_weighted:
        w = torch_ref.task_weights(states[:, -num_tasks:],
                                   log_alpha_det.exp()).unsqueeze(-1)
        l1, l2 = w * l1, w * l2
    return l1.mean(), l2.mean()


class _ActorAlphaLoss(torch.autograd.Function):
    """(actor_loss, alpha_loss, entropy) fused.

    actor_loss = mean/weighted of -(min(q1,q2) - alpha_i * logp)
    alpha_loss = -mean(log_alpha[t_i] * (logp.detach() + H_bar))
    entropy    = mean(0.5*A*(1+log 2pi) + sum log_std)   [diagnostic]

    Gradients: actor_loss -> q1,q2,logp; alpha_loss -> log_alpha.
    (alpha is detached in the actor loss and logp in the alpha loss —
    reference learner.py:316, model.py:80-116.)
    """

    @staticmethod
    def forward(ctx, q1, q2, logp, log_stds, states, log_alpha,
                num_tasks: int, use_weighted: bool, H_bar: float):
        ext = native()
        out = ext.actor_alpha_loss_fwd(
            q1.contiguous(), q2.contiguous(), logp.contiguous(),
            log_stds.contiguous(), states.contiguous(), log_alpha.detach(),
            num_tasks, int(use_weighted), H_bar)
        ctx.save_for_backward(q1, q2, logp, states, log_alpha.detach(), out)
        ctx.meta = (num_tasks, use_weighted, H_bar)
        actor_l, alpha_l, entropy = out[0], out[2], out[3]
        ctx.mark_non_differentiable(entropy)
        return actor_l, alpha_l, entropy

    @staticmethod
    def backward(ctx, gp, gal, _gent):
        q1, q2, logp, states, la, saved = ctx.saved_tensors
        T, use_w, H_bar = ctx.meta
        gscale = torch.stack([gp.reshape(()), gal.reshape(())]).contiguous()
        daq1, daq2, dlp, dla = native().actor_alpha_loss_bwd(
            q1.contiguous(), q2.contiguous(), logp.contiguous(),
            states.contiguous(), la, saved, gscale, T, int(use_w), H_bar)
        return daq1, daq2, dlp, None, None, dla, None, None, None


def actor_alpha_loss(q1, q2, logp, log_stds, states, log_alpha, num_tasks,
                     use_weighted, H_bar):
    """Returns (actor_loss, alpha_loss, entropy)."""
    if _use_native(q1):
        return _ActorAlphaLoss.apply(q1, q2, logp, log_stds, states,
                                     log_alpha, num_tasks, use_weighted,
                                     float(H_bar))
    qmin = torch.min(q1, q2)
    if num_tasks > 1:
        one_hots = states[:, -num_tasks:]
        alpha = torch_ref.gather_log_alpha(one_hots,
                                           log_alpha).exp().detach()
        la_g = torch_ref.gather_log_alpha(one_hots, log_alpha)
    else:
        alpha = log_alpha.exp().detach()
        la_g = log_alpha
    pl = -(qmin - alpha * logp)
    if use_weighted:
        w = torch_ref.task_weights(states[:, -num_tasks:],
                                   log_alpha.exp().detach()).unsqueeze(-1)
        pl = w * pl
    actor_loss = pl.mean()
    alpha_loss = -(la_g * (logp.detach() + H_bar)).mean()
    entropy = torch_ref.entropy_from_log_std(log_stds)
    return actor_loss, alpha_loss, entropy


# ---------------------------------------------------------------------------
# Non-differentiable / glue ops
# ---------------------------------------------------------------------------

def td_target(rewards, dones, q1_t, q2_t, next_logp, alpha, gamma, reward_scale):
    if _use_native(rewards) and has_native():
        alpha_t = alpha if torch.is_tensor(alpha) else torch.full_like(rewards, float(alpha))
        if alpha_t.numel() == 1:
            alpha_t = alpha_t.expand_as(rewards).contiguous()
        return native().td_target(rewards, dones, q1_t, q2_t, next_logp,
                                  alpha_t, float(gamma), float(reward_scale))
    return torch_ref.td_target(rewards, dones, q1_t, q2_t, next_logp,
                               alpha, gamma, reward_scale)


def polyak_(target_params, source_params, tau: float) -> None:
    tps = list(target_params)
    sps = list(source_params)
    if tps and _use_native(tps[0]) and len(tps) == 1:
        native().polyak_(tps[0], sps[0], float(tau))
        return
    torch_ref.polyak_(tps, sps, tau)


# Pure-torch glue (tiny matmuls/reductions — not worth custom kernels; the
# heavy path is the fused MLP/squash/Adam/Polyak kernels):
task_weights = torch_ref.task_weights
gather_log_alpha = torch_ref.gather_log_alpha
entropy_from_log_std = torch_ref.entropy_from_log_std
batched_linear = torch_ref.batched_linear
attention_pool = torch_ref.attention_pool


# ---------------------------------------------------------------------------
# bf16 mixed-precision GEMM paths (fp32 master weights + bf16 compute
# mirrors; fp32 accumulation and fp32 weight grads).  The bf16 mirrors ride
# along as non-tracked args; the fp32 parameters are the autograd inputs so
# dW/db accumulate into the flat fp32 gradient buffers.
# ---------------------------------------------------------------------------

class _MLPBF16(torch.autograd.Function):
    """Whole-MLP fused forward/backward on the bf16 GEMM kernels, for G
    networks at once (grid.z = G).  Layer 0 consumes the shared x; later
    layers run per group on [G,B,*]; the output is fp32.  As in _MLPF32,
    G == 1 has no group dimension and the layer-0 dX is summed over the
    groups.  The ReLU masks come from the saved bf16 hidden outputs.

    transposed: the CARE mixture of k encoders.  The fp32 parameters are
    the reference's batched-Linear W (k,in,out) / b (k,1,out)
    (state_encoder.Linear); compute uses TRANSPOSED bf16 mirrors (k,out,in)
    matching the GEMM kernel's [G,N,K] layout, so dW goes back permuted.
    Its consumer weighs the stacked [k,B,out] as one tensor; the twin
    critic (G > 1, not transposed) returns one output per head.  The
    mixture's backward runs full-batch (grad_row_start=0: upstream grads
    are zero outside the grad-carrying rows; the mixture layers are 50-wide
    — cheaper than slicing per-group activations contiguous).
    """

    @staticmethod
    def forward(ctx, x: torch.Tensor, n_layers: int, G: int,
                grad_row_start: int, transposed: bool, ws_bf16, *wb_f32):
        ext = native()
        bs = wb_f32[n_layers:]
        acts = [x.to(torch.bfloat16)]
        for i in range(n_layers):
            last = i == n_layers - 1
            b = bs[i].view(G, -1) if transposed else bs[i]
            acts.append(ext.linear_act_fwd_bf16(
                acts[-1], ws_bf16[i], b.contiguous(),
                ACT_NONE if last else ACT_RELU, G, 1 if last else 0))
        h = acts.pop()          # fp32
        ctx.save_for_backward(*acts)     # bf16: input + hidden outputs
        ctx.ws_bf16 = ws_bf16
        ctx.n_layers = n_layers
        ctx.G = G
        ctx.grad_row_start = grad_row_start
        ctx.transposed = transposed
        if G == 1 or transposed:
            return h
        return tuple(h[g] for g in range(G))

    @staticmethod
    def backward(ctx, *grads: torch.Tensor):
        n, G = ctx.n_layers, ctx.G
        acts = list(ctx.saved_tensors)
        ws = ctx.ws_bf16
        ext = native()
        # forward args: (x, n_layers, G, grad_row_start, transposed,
        # ws_bf16, *ws_f32, *bs_f32) — the non-tensor arguments always
        # report False, so the weights are counted from the end
        need_w = ctx.needs_input_grad[-2 * n:-n]
        dy = grads[0] if len(grads) == 1 else torch.stack(grads, dim=0)
        r0 = ctx.grad_row_start
        if r0:
            acts = [a[..., r0:, :] for a in acts]
            dy = dy[..., r0:, :]
        dy = dy.contiguous().to(torch.bfloat16)
        dx = None
        dws: List[Optional[torch.Tensor]] = [None] * n
        dbs: List[Optional[torch.Tensor]] = [None] * n
        for i in range(n - 1, -1, -1):
            act = ACT_RELU if i < n - 1 else ACT_NONE
            yout = acts[i + 1] if i < n - 1 else acts[i]  # dummy when act=0
            if need_w[i]:
                dw, db = ext.linear_bwd_dwdb_bf16(dy, acts[i], yout, act, G)
                if ctx.transposed:
                    dw, db = dw.permute(0, 2, 1), db.view(G, 1, -1)
                dws[i], dbs[i] = dw, db
            if i > 0:
                dy = ext.linear_bwd_dx_bf16(dy, ws[i], yout, act, G, 0)
            elif ctx.needs_input_grad[0]:
                dx = ext.linear_bwd_dx_bf16(dy, ws[0], yout, act, G,
                                            1).to(torch.float32)
        return (dx, None, None, None, None, None, *dws, *dbs)


def mlp_forward_bf16(x, ws_f32, bs_f32, ws_bf16, grad_row_start: int = 0):
    return _MLPBF16.apply(x, len(ws_f32), 1, grad_row_start, False,
                          tuple(ws_bf16), *ws_f32, *bs_f32)


def twin_mlp_forward_bf16(x, stacked_ws_f32, stacked_bs_f32, ws_bf16):
    return _MLPBF16.apply(x, len(ws_bf16), 2, 0, False, tuple(ws_bf16),
                          *stacked_ws_f32, *stacked_bs_f32)


def grouped_mlp_bf16(x, W_f32_list, b_f32_list, ws_bf16T_list, k: int):
    """CARE mixture-of-k-encoders as grouped bf16 GEMMs: [k,B,out] fp32."""
    return _MLPBF16.apply(x, len(W_f32_list), k, 0, True,
                          tuple(ws_bf16T_list), *W_f32_list, *b_f32_list)
