"""Pure-torch fp32 reference implementations of every hot-path op.

These are (a) the CPU execution path, (b) the numerics oracle the HIP
kernels are unit-tested against, and (c) the executable spec of the
reference's math:

- :func:`mlp_forward`        — reference ``build_mlp`` products
  (MT10_Distributed_MTSAC/src/utils.py:36-57) / LL Actor/Critic forward
  (LunarLander_Distributed_SAC/src/model.py:41-44,120-125).
- :func:`squashed_gaussian`  — tanh-squashed Gaussian rsample + log-prob
  (LunarLander…/src/model.py:45-59; MT10…MTSAC/src/model.py:43-56).
- :func:`td_target`          — Bellman backup
  (LunarLander…/src/learner.py:206-210; MT10…MTSAC/src/learner.py:270-276).
- :func:`task_weights`       — per-task weighted-loss weights
  (MT10_Distributed_MTSAC/src/model.py:99-116,177-196).
- :func:`gather_log_alpha`   — per-sample alpha (MT10…MTSAC/src/learner.py:213-233).
- :func:`entropy_from_log_std` — diagnostic entropy
  (MT10…MTSAC/src/learner.py:311-312).
- :func:`polyak_`            — soft target update (learner.soft_update).

All math is fp32 (the reference never uses mixed precision); the HIP path
may run GEMMs in bf16-in/fp32-accumulate and is tested against these at
bf16-appropriate tolerances.
"""

from __future__ import annotations

import math
from typing import Iterable, Optional, Sequence

import torch
import torch.nn.functional as F

LOG_STD_MIN = -20.0
LOG_STD_MAX = 2.0
_LOG_SQRT_2PI = 0.5 * math.log(2 * math.pi)


def mlp_forward(x: torch.Tensor,
                weights: Sequence[torch.Tensor],
                biases: Sequence[torch.Tensor],
                final_act: Optional[str] = None) -> torch.Tensor:
    """ReLU MLP: hidden layers ReLU-activated, output layer linear.

    Matches reference ``build_mlp`` semantics (hidden Linear+ReLU stack, no
    output activation — MT10…MTSAC/src/utils.py:36-57).
    """
    n = len(weights)
    for i, (w, b) in enumerate(zip(weights, biases)):
        x = F.linear(x, w, b)
        if i < n - 1:
            x = torch.relu(x)
        elif final_act == "relu":
            x = torch.relu(x)
    return x


def squashed_gaussian(mu: torch.Tensor, log_std: torch.Tensor,
                      eps: torch.Tensor, k: float):
    """Tanh-squashed Gaussian sample + summed log-prob.

    Given pre-clamp log_std, applies the reference clamp to [-20, 2]
    (model.forward), then u = mu + std*eps, a = k*tanh(u),
    logp = sum_i [ logN(u_i; mu_i, std_i) - log(k*(1 - tanh(u_i)^2 + 1e-6)) ]
    (reference model.get_action_log_prob…, LunarLander…/src/model.py:51-59).

    Returns (action, log_prob[B,1], log_std_clamped).
    """
    log_std = torch.clamp(log_std, LOG_STD_MIN, LOG_STD_MAX)
    std = torch.exp(log_std)
    u = mu + std * eps
    t = torch.tanh(u)
    action = k * t
    gaussian_log_prob = -0.5 * eps.pow(2) - log_std - _LOG_SQRT_2PI
    log_prob = gaussian_log_prob - torch.log(k * (1 - t.pow(2) + 1e-6))
    return action, log_prob.sum(dim=-1, keepdim=True), log_std


def td_target(rewards: torch.Tensor, dones: torch.Tensor,
              q1_target: torch.Tensor, q2_target: torch.Tensor,
              next_log_probs: torch.Tensor, alpha: torch.Tensor,
              gamma: float, reward_scale: float) -> torch.Tensor:
    """y = scale*r + gamma*(1-d)*(min(Q1t,Q2t) - alpha*logp') — reference
    learner.update_SAC (MT10…MTSAC/src/learner.py:270-276)."""
    return reward_scale * rewards + gamma * (1 - dones) * (
        torch.min(q1_target, q2_target) - alpha * next_log_probs)


def task_weights(one_hots: torch.Tensor, alphas: torch.Tensor) -> torch.Tensor:
    """Per-sample weights for the weighted multi-task loss.

    w_i = softmax(-alpha)[task(i)], renormalized to sum to 1 over the batch
    (reference MT10_Distributed_MTSAC/src/model.py:99-116).  ``alphas`` is
    exp(log_alpha).detach() of shape (num_tasks,).
    """
    task_indices = torch.argmax(one_hots, dim=1)
    w = F.softmax(-alphas, dim=0)[task_indices].detach()
    return w / w.sum()


def gather_log_alpha(one_hots: torch.Tensor, log_alpha: torch.Tensor) -> torch.Tensor:
    """(B, num_tasks) @ (num_tasks, 1) -> (B, 1) per-sample log_alpha
    (reference MT10…MTSAC/src/learner.py:213-233)."""
    return torch.matmul(one_hots, log_alpha.unsqueeze(0).t())


def entropy_from_log_std(log_std: torch.Tensor) -> torch.Tensor:
    """Mean analytic Gaussian entropy: 0.5*d*(1+ln 2pi) + sum(log_std)
    (reference MT10…MTSAC/src/learner.py:311-312)."""
    d = log_std.shape[1]
    return (0.5 * d * (1.0 + math.log(2 * math.pi))
            + log_std.sum(dim=-1)).mean()


@torch.no_grad()
def polyak_(target_params: Iterable[torch.Tensor],
            source_params: Iterable[torch.Tensor], tau: float) -> None:
    """theta_target <- tau*theta + (1-tau)*theta_target (reference
    learner.soft_update; tau=1.0 is the hard copy)."""
    for tp, sp in zip(target_params, source_params):
        tp.mul_(1.0 - tau).add_(sp, alpha=tau)


# ---------------------------------------------------------------------------
# CARE mixture-of-encoders + attention pool (reference
# MT10_Distributed_CARE/src/state_encoder.py:85-94,146-174).
# ---------------------------------------------------------------------------

def batched_linear(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """k parallel Linear layers: w (k,in,out), b (k,1,out).

    x (B,in) -> (k,B,out), or x (k,B,in) -> (k,B,out) — the reference's
    einsum pair ('kio,bi->kbo' / 'kio,kbi->kbo',
    MT10_Distributed_CARE/src/state_encoder.py:146-174).
    """
    if x.dim() == 2:
        return torch.einsum("kio,bi->kbo", w, x) + b
    return torch.einsum("kio,kbi->kbo", w, x) + b


def attention_pool(z_encs: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
    """softmax(logits) convex combination of per-encoder embeddings.

    z_encs (B,k,D), logits (B,k) -> (B,D)
    (reference state_encoder.py:85-89).
    """
    alpha = F.softmax(logits, dim=-1)
    return (z_encs * alpha.unsqueeze(-1)).sum(dim=1)


# ---------------------------------------------------------------------------
# Packed replay ingest (docs/KERNELS.md "packed replay batch"): CPU path and
# oracle of the k_replay_ingest scatter kernel.
# ---------------------------------------------------------------------------

PK_HDR = 4    # header words: n_desc, T, total_rows, used
PK_DESC = 8   # words per descriptor:
#               task, n, first, rows, offset, dst_row, row_base, 0


def packed_header_words(num_tasks: int, max_desc: int) -> int:
    """Words reserved in front of the payloads for ``max_desc`` blocks."""
    return PK_HDR + num_tasks + PK_DESC * max_desc


def packed_validate(packed: torch.Tensor, num_tasks: int, cap: int,
                    state_dim: int, action_dim: int) -> list:
    """Check every header field of a packed batch against the replay
    geometry and the buffer's own extent; returns the descriptors as
    rows of ints.  Raises ``ValueError`` on the first bad field — a bad
    descriptor must never reach a scatter."""
    if packed.device.type != "cpu" or packed.dtype != torch.float32 \
            or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError("packed batch must be a flat fp32 host tensor")
    T = num_tasks
    if packed.numel() < PK_HDR + T:
        raise ValueError("packed header truncated")
    h = packed.view(torch.int32)
    n_desc, t_hdr, total_rows, used = h[:PK_HDR].tolist()
    if t_hdr != T:
        raise ValueError("packed batch built for another task count")
    pay0 = PK_HDR + T + PK_DESC * n_desc
    if n_desc < 1 or pay0 > packed.numel():
        raise ValueError("packed descriptor count out of range")
    if used < pay0 or used > packed.numel():
        raise ValueError("packed batch larger than the staging buffer")
    for s in packed[PK_HDR:PK_HDR + T].tolist():
        if not 0.0 <= s <= float(cap):
            raise ValueError("packed size outside [0, cap]")
    descs = h[PK_HDR + T:pay0].reshape(n_desc, PK_DESC).tolist()
    row_floats = 2 * state_dim + action_dim + 2
    per_task = [0] * T
    base = 0
    for task, n, first, rows, off, dst, row_base, _ in descs:
        if not 0 <= task < T:
            raise ValueError("packed descriptor: task out of range")
        if n < 1 or rows < 1 or rows > cap or first < 0 or first + rows > n:
            raise ValueError("packed descriptor: rows out of range")
        if off < pay0 or off + n * row_floats > used:
            raise ValueError(
                "packed descriptor: payload outside the staging buffer")
        if not 0 <= dst < cap:
            raise ValueError("packed descriptor: bad dst row")
        if row_base != base:
            raise ValueError("packed descriptor: bad row_base")
        base += rows
        per_task[task] += rows
        if per_task[task] > cap:
            raise ValueError(
                "packed batch aliases rows of one task (rows > cap)")
    if base != total_rows:
        raise ValueError("packed row total disagrees")
    return descs


@torch.no_grad()
def replay_ingest(packed: torch.Tensor, states: torch.Tensor,
                  actions: torch.Tensor, rewards: torch.Tensor,
                  next_states: torch.Tensor, dones: torch.Tensor,
                  sizes: torch.Tensor) -> int:
    """Decode one packed batch into the ``[T, cap, D]`` field tensors and
    the per-task ``sizes``.  Validates first (nothing is written when a
    descriptor is bad).  Returns the number of rows written."""
    T, cap, Ds = states.shape
    Da = actions.shape[2]
    descs = packed_validate(packed, T, cap, Ds, Da)
    total = 0
    for task, n, first, rows, off, dst, _base, _ in descs:
        p = packed[off:off + n * (2 * Ds + Da + 2)]
        o = 0
        src = []
        for w in (Ds, Da, 1, Ds, 1):
            src.append(p[o:o + n * w].reshape(n, w)[first:first + rows])
            o += n * w
        idx = (torch.arange(rows) + dst) % cap
        for field, s in zip((states, actions, rewards, next_states, dones),
                            src):
            field[task].index_copy_(0, idx.to(field.device),
                                    s.to(field.device))
        total += rows
    sizes.copy_(packed[PK_HDR:PK_HDR + T])
    return total


# ---------------------------------------------------------------------------
# Without-replacement replay draw (docs/KERNELS.md "replay permutation"): the
# CPU path and the exact oracle of k_replay_sample_norepl.  Same integer
# algorithm, in int64 tensors: additions and multiplications wrap like the
# kernel's uint64, right shifts are made logical by masking.
# ---------------------------------------------------------------------------

NR_ROUNDS = 8        # Feistel rounds
NR_MIN_BITS = 6      # floor of the permutation's domain width


def _i64(x: int) -> int:
    """A 64-bit word as the signed Python int with the same bits."""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= (1 << 63) else x


def _lsr(x: torch.Tensor, k: int) -> torch.Tensor:
    return (x >> k) & ((1 << (64 - k)) - 1)


def _sm64(x: torch.Tensor) -> torch.Tensor:
    """splitmix64 finalizer on int64 bit patterns (the kernels' dsac_sm64)."""
    x = x + _i64(0x9E3779B97F4A7C15)
    x = (x ^ _lsr(x, 30)) * _i64(0xBF58476D1CE4E5B9)
    x = (x ^ _lsr(x, 27)) * _i64(0x94D049BB133111EB)
    return x ^ _lsr(x, 31)


@torch.no_grad()
def norepl_index(n: torch.Tensor, t: torch.Tensor, j: torch.Tensor,
                 ctr: torch.Tensor, return_walk: bool = False):
    """Elementwise ``(P_key(j mod n) + rot_key) mod n`` for int64 tensors
    of one shape: shard sizes ``n`` (>= 1), shard numbers ``t``, row
    positions ``j`` and rng counters ``ctr``.  ``P_key`` is ``NR_ROUNDS``
    alternating unbalanced XOR-Feistel rounds over ``max(NR_MIN_BITS,
    ceil(log2 n))`` bits, cycle-walked into ``[0, n)``.  With
    ``return_walk`` also returns how many times each element applied the
    network."""
    n, t, j, ctr = (v.contiguous()
                    for v in torch.broadcast_tensors(n, t, j, ctr))
    key = _sm64(ctr * 0x100000001 + _i64(1 << 63) + t)
    rot = _lsr(_sm64(key), 32) % n
    b = torch.full_like(n, NR_MIN_BITS)
    for k in range(NR_MIN_BITS, 32):   # ceil(log2 n) = #{k : 2^k < n}
        b += (n > (1 << k)).to(b.dtype)
    bl = b >> 1
    one = torch.ones_like(n)
    ml = (one << bl) - 1
    mh = (one << (b - bl)) - 1
    x = j % n
    walk = torch.zeros_like(n)
    todo = torch.ones_like(n, dtype=torch.bool)
    while bool(todo.any()):
        lo, hi = x & ml, x >> bl
        for r in range(NR_ROUNDS):
            kr = key + ((r + 1) << 32)
            if r % 2 == 0:
                lo = lo ^ (_lsr(_sm64(kr + hi), 32) & ml)
            else:
                hi = hi ^ (_lsr(_sm64(kr + lo), 32) & mh)
        x = torch.where(todo, (hi << bl) | lo, x)
        walk += todo.to(walk.dtype)
        todo = todo & (x >= n)
    idx = (x + rot) % n
    return (idx, walk) if return_walk else idx


@torch.no_grad()
def replay_sample_indices_norepl(sizes, B: int, T: int, ctr) -> torch.Tensor:
    """In-shard indices of a stratified without-replacement draw: int64
    ``[T * (B // T)]``, rows ``t * per .. (t + 1) * per - 1`` from shard
    ``t``.  ``sizes`` holds the T shard sizes (tensor or sequence; an empty
    shard yields index 0), ``ctr`` the rng counter (int or one-element
    tensor).  Rows of one shard are distinct whenever its size is at least
    ``per``; a smaller shard repeats its rows as evenly as possible."""
    sizes = torch.as_tensor(sizes)
    dev = sizes.device
    per = int(B) // int(T)
    n = sizes.reshape(-1)[:T].to(torch.int64).clamp(min=1)
    if not torch.is_tensor(ctr):
        ctr = torch.tensor(_i64(int(ctr)), dtype=torch.int64)
    c = ctr.reshape(-1)[:1].to(device=dev, dtype=torch.int64)
    t = torch.arange(T, device=dev, dtype=torch.int64)
    j = torch.arange(per, device=dev, dtype=torch.int64)
    return norepl_index(n[:, None], t[:, None], j[None, :],
                        c[None, :]).reshape(-1)


# ---------------------------------------------------------------------------
# Prioritized replay (docs/KERNELS.md "Prioritized replay"): the CPU path and
# the exact oracle of k_replay_sample_per, k_critic_td_loss_per's priorities,
# the write-back kernels and the ingest hook.  State of a replay with T
# shards of ``cap`` rows: leaves ``prio [T, cap]`` (0 = never written), block
# sums ``bsum [T, ceil(cap / PER_BLOCK)]``, ``total [T]``, ``max_prio [T]``.
# Sums are only ever recomputed from what they cover, in one fixed order.
# ---------------------------------------------------------------------------

PER_BLOCK = 1024     # leaves per block sum


def per_fixed_sum(v: torch.Tensor) -> torch.Tensor:
    """Sum over the last dim in the kernels' fixed order: 256 strided
    partials (element i, i + 256, i + 512, ... added in that order), folded
    by halves (i with i + 128, then + 64, ... + 1)."""
    n = v.shape[-1]
    v = F.pad(v, (0, (-n) % 256)).reshape(*v.shape[:-1], -1, 256)
    acc = v[..., 0, :]
    for k in range(1, v.shape[-2]):
        acc = acc + v[..., k, :]
    h = 128
    while h >= 1:
        acc = acc[..., :h] + acc[..., h:2 * h]
        h //= 2
    return acc[..., 0]


def per_resum(prio: torch.Tensor):
    """``(bsum, total)`` of leaves ``prio [T, cap]`` — the invariant every
    prioritized-replay kernel maintains, bit for bit."""
    T, cap = prio.shape
    nb = (cap + PER_BLOCK - 1) // PER_BLOCK
    leaves = F.pad(prio, (0, nb * PER_BLOCK - cap)).reshape(T, nb, PER_BLOCK)
    bsum = per_fixed_sum(leaves)
    return bsum, per_fixed_sum(bsum)


def _hs_scan64(v: torch.Tensor) -> torch.Tensor:
    """Hillis-Steele inclusive scan over a last dim of 64 (the wave scan of
    the kernel: element l adds element l - off for off = 1, 2, ... 32)."""
    for off in (1, 2, 4, 8, 16, 32):
        v = torch.cat([v[..., :off], v[..., off:] + v[..., :-off]], dim=-1)
    return v


def _per_prefix(p: torch.Tensor) -> torch.Tensor:
    """Inclusive prefix sums over the last dim as the kernel forms them:
    chunks of 64, a wave scan each, plus the running base."""
    n = p.shape[-1]
    c = F.pad(p, (0, (-n) % 64)).reshape(*p.shape[:-1], -1, 64)
    sc = _hs_scan64(c)
    base = torch.zeros(p.shape[:-1], dtype=p.dtype, device=p.device)
    out = []
    for k in range(sc.shape[-2]):
        incl = base[..., None] + sc[..., k, :]
        out.append(incl)
        base = incl[..., 63]
    return torch.cat(out, dim=-1)[..., :n]


def _per_search(p: torch.Tensor, x: torch.Tensor):
    """Per row of ``p [R, n]``: the first k with ``p[k] > 0`` whose inclusive
    prefix exceeds ``x [R]`` and the prefix before it; where there is none
    (rounding), the last k with ``p[k] > 0`` (0 if none).  Returns
    ``(k, excl, found)``."""
    n = p.shape[-1]
    incl = _per_prefix(p)
    ar = torch.arange(n, device=p.device).expand_as(p)
    hit = (incl > x[:, None]) & (p > 0)
    found = hit.any(dim=-1)
    first = torch.where(hit, ar, torch.full_like(ar, n)).min(dim=-1).values
    last = torch.where(p > 0, ar, torch.full_like(ar, -1)).max(dim=-1).values
    k = torch.where(found, first, last.clamp(min=0))
    prev = incl.gather(1, (k - 1).clamp(min=0)[:, None])[:, 0]
    excl = torch.where(k > 0, prev, torch.zeros_like(prev))
    return k, excl, found


def per_uniforms(B: int, ctr) -> torch.Tensor:
    """The (0, 1) uniform k_replay_sample derives from the rng counter for
    each of the B batch rows (fp32)."""
    if not torch.is_tensor(ctr):
        ctr = torch.tensor(_i64(int(ctr)), dtype=torch.int64)
    c = ctr.reshape(-1)[:1].to(device="cpu", dtype=torch.int64)
    i = torch.arange(B, dtype=torch.int64)
    h = _sm64(c * 0x100000001 + i * 2 + 2)
    u = (_lsr(h, 40) + 1).to(torch.float32) * 5.9604644775390625e-8
    return torch.where(u < 1.0, u, torch.full_like(u, 0.99999994))


@torch.no_grad()
def per_sample_indices(prio: torch.Tensor, bsum: torch.Tensor,
                       total: torch.Tensor, sizes, B: int, T: int, ctr,
                       return_x: bool = False):
    """In-shard indices of one stratified proportional draw: int64
    ``[T * (B // T)]``, rows ``t * per .. (t + 1) * per - 1`` from shard t.
    Row j of a shard draws at ``x = (float(j) + u) * (total_t / float(per))``
    (fp32, in that order; ``u`` from :func:`per_uniforms`) and takes the
    first row whose inclusive prefix sum of the priorities exceeds x — first
    the block, over ``bsum``, then the leaf, over the block's leaves and x
    minus the prefix before the block.  Rounding: if no block (leaf)
    qualifies, the last one with a non-zero sum (priority) is taken; a row
    with zero priority is never taken.  An empty shard yields 0."""
    dev = prio.device
    per = int(B) // int(T)
    cap = prio.shape[1]
    nb = bsum.shape[1]
    sizes = torch.as_tensor(sizes, dtype=torch.float32, device=dev) \
        .reshape(-1)[:T].clamp(max=float(cap))
    u = per_uniforms(per * T, ctr).to(dev).reshape(T, per)
    j = torch.arange(per, dtype=torch.float32, device=dev)
    tot = total.reshape(-1)[:T].to(torch.float32)
    x = (j[None, :] + u) * (tot / float(per))[:, None]
    leaves = F.pad(prio, (0, nb * PER_BLOCK - cap)).reshape(T, nb, PER_BLOCK)
    idx = torch.zeros(T, per, dtype=torch.int64, device=dev)
    for t in range(T):
        if not (float(sizes[t]) >= 1.0 and float(tot[t]) > 0.0):
            continue
        b, excl, found = _per_search(bsum[t].expand(per, nb), x[t])
        xr = torch.where(found, x[t] - excl,
                         torch.full_like(excl, float("inf")))
        k, _, _ = _per_search(leaves[t][b], xr)
        idx[t] = b * PER_BLOCK + k
    idx = idx.reshape(-1)
    return (idx, x.reshape(-1)) if return_x else idx


@torch.no_grad()
def per_is_weights(prio: torch.Tensor, total: torch.Tensor, sizes,
                   idx: torch.Tensor, beta) -> torch.Tensor:
    """Raw importance-sampling weights ``(n_t * p_i / total_t) ** -beta`` of
    the in-shard indices ``idx [T * per]`` (shard-major); 1 for an empty
    shard or a zero priority."""
    T, cap = prio.shape
    dev = prio.device
    per = idx.numel() // T
    n = torch.as_tensor(sizes, dtype=torch.float32, device=dev) \
        .reshape(-1)[:T].clamp(max=float(cap))
    beta = torch.as_tensor(beta, dtype=torch.float32, device=dev).reshape(-1)[0]
    p = prio.gather(1, idx.reshape(T, per))
    tot = total.reshape(-1)[:T, None]
    ok = (n[:, None] >= 1.0) & (tot > 0.0) & (p > 0.0)
    ratio = torch.where(ok, n[:, None] * p / tot, torch.ones_like(p))
    return torch.pow(ratio, -beta).reshape(-1)


def per_new_priorities(d1: torch.Tensor, d2: torch.Tensor, alpha: float,
                       eps: float) -> torch.Tensor:
    """``(0.5 (|d1| + |d2|) + eps) ** alpha`` of the two TD errors."""
    return torch.pow(0.5 * (d1.abs() + d2.abs()) + eps, alpha).reshape(-1)


def _per_resum_blocks(prio, bsum, total, t: int, rows: torch.Tensor) -> None:
    """Re-sum the blocks of shard t holding ``rows`` and the shard total."""
    cap = prio.shape[1]
    for b in torch.unique(rows // PER_BLOCK).tolist():
        leaf = prio[t, b * PER_BLOCK:min(cap, (b + 1) * PER_BLOCK)]
        bsum[t, b] = per_fixed_sum(leaf)
    total[t] = per_fixed_sum(bsum[t])


@torch.no_grad()
def per_update_(prio: torch.Tensor, bsum: torch.Tensor, total: torch.Tensor,
                max_prio: torch.Tensor, idx: torch.Tensor,
                new_prio: torch.Tensor) -> None:
    """Write-back: every row of the flat indices ``idx`` (``t * cap + row``)
    takes its new priority, a row listed more than once the MAXIMUM of its
    values; ``max_prio[t]`` is raised to the largest value written; touched
    blocks and the totals are re-summed.  A value that is not positive
    (NaN included) counts as 0."""
    T, cap = prio.shape
    idx = idx.reshape(-1).to(torch.int64)
    v = new_prio.reshape(-1).to(torch.float32)
    v = torch.where(v > 0, v, torch.zeros_like(v))
    flat = prio.reshape(-1)
    flat[idx] = 0.0
    flat.scatter_reduce_(0, idx, v, reduce="amax", include_self=True)
    t_of = idx // cap
    max_prio.scatter_reduce_(0, t_of, v, reduce="amax", include_self=True)
    for t in torch.unique(t_of).tolist():
        _per_resum_blocks(prio, bsum, total, t, idx[t_of == t] - t * cap)


@torch.no_grad()
def per_ingest_(prio: torch.Tensor, bsum: torch.Tensor, total: torch.Tensor,
                max_prio: torch.Tensor, t: int, start: int, rows: int) -> None:
    """Ingest hook: rows ``[start, start + rows) mod cap`` of shard t receive
    ``max_prio[t]``; touched blocks and the shard total are re-summed."""
    cap = prio.shape[1]
    if rows <= 0:
        return
    r = (torch.arange(min(int(rows), cap), device=prio.device)
         + int(start)) % cap
    prio[t, r] = max_prio[t]
    _per_resum_blocks(prio, bsum, total, t, r)


# ---------------------------------------------------------------------------
# Gradient-norm clipping (docs/KERNELS.md "Gradient-norm clipping").
# ---------------------------------------------------------------------------

def check_max_grad_norm(v):
    """``None`` (off) or a positive number, ``inf`` included (guard and
    metrics only); anything else raises ValueError.  Returns a float."""
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(f"max_grad_norm must be a positive number, got {v!r}")
    v = float(v)
    if not v > 0.0:   # also NaN
        raise ValueError(f"max_grad_norm must be a positive number, got {v!r}")
    return v


@torch.no_grad()
def grad_clip_coef(g: torch.Tensor, max_norm: float):
    """``(s, norm, coef, ok)`` of one flat fp32 gradient, as 0-d tensors:
    ``s = sum g_i^2``, ``norm = sqrt(s)``, ``ok = isfinite(s)`` and
    ``coef = min(1, max_norm / (norm + 1e-6))`` — the formula of
    ``torch.nn.utils.clip_grad_norm_`` — or 0 where the step is skipped."""
    g = g.reshape(-1).to(torch.float32)
    s = (g * g).sum()
    # correctly rounded, as sqrtf (torch's fp32 CPU sqrt is not always)
    norm = s.double().sqrt().float()
    ok = torch.isfinite(s)
    # fp32 operands throughout: the kernel's arithmetic, bit for bit
    c, tiny = (torch.tensor(x, dtype=torch.float32, device=g.device)
               for x in (float(max_norm), 1e-6))
    coef = torch.where(ok, (c / (norm + tiny)).clamp(max=1.0),
                       torch.zeros_like(norm))
    return s, norm, coef, ok


# ---------------------------------------------------------------------------
# bf16 MFMA GEMM oracle (docs/KERNELS.md "Numerics").  Every GEMM kernel
# takes bf16 operands (exact in float64), forms exact products, adds them in
# fp32 in an order the hardware does not specify, and rounds once at the
# end.  So the check is an inequality: with ``n`` accumulated terms and
# ``mag = sum |a| |w| (+ |bias|)``, any order of n fp32 additions stays
# within ``(n + 2) * 2^-23 * mag`` of the exact sum — one whole ulp per
# addition, so an adder that truncates satisfies it too — plus a floor for
# a flushed denormal.  A bf16 output adds its own rounding, unit roundoff
# 2^-8.  Feeding each layer the kernel's own saved bf16 input ("teacher
# forcing") makes every layer one such GEMM with exactly known operands.
# ---------------------------------------------------------------------------

GEMM_ULP = 2.0 ** -23       # one fp32 ulp (relative) per addition
GEMM_FLOOR = 2.0 ** -100    # a flushed denormal
BF16_ROUNDOFF = 2.0 ** -8   # unit roundoff of bf16 (8 significant bits)


@torch.no_grad()
def gemm_oracle(a: torch.Tensor, w: torch.Tensor,
                bias: Optional[torch.Tensor] = None, relu: bool = False,
                mask: Optional[torch.Tensor] = None,
                n: Optional[int] = None):
    """``(ref, tol)`` in float64 of ``a [..., M, K] @ w [..., N, K]^T``
    (+ ``bias [..., N]``), ReLU and ``mask`` (False = forced to exactly 0)
    applied in float64.  ``n`` is the number of accumulated terms (default
    K; rows plus partials for a split-K sum, every term for a sum over
    groups).  ``tol = (n + 2) * 2^-23 * mag + 2^-100``; where the mask
    forces a zero, ``tol`` is 0."""
    a64, w64 = a.double(), w.double()
    ref = a64 @ w64.transpose(-1, -2)
    mag = a64.abs() @ w64.abs().transpose(-1, -2)
    if bias is not None:
        b64 = bias.double().unsqueeze(-2)
        ref = ref + b64
        mag = mag + b64.abs()
    if n is None:
        n = a.shape[-1]
    tol = (n + 2) * GEMM_ULP * mag + GEMM_FLOOR
    if relu:
        ref = ref.clamp(min=0.0)     # |relu(x) - relu(y)| <= |x - y|
    if mask is not None:
        ref = torch.where(mask, ref, torch.zeros_like(ref))
        tol = torch.where(mask, tol, torch.zeros_like(tol))
    return ref, tol


@torch.no_grad()
def gemm_bound_ratio(out: torch.Tensor, ref: torch.Tensor,
                     tol: torch.Tensor) -> torch.Tensor:
    """Elementwise ``err / bound`` of a kernel output against
    :func:`gemm_oracle`: the bound is ``tol`` for an fp32 output and
    ``tol + 2^-8 (|ref| + tol)`` for a bf16 one.  An element within its
    bound yields a ratio in [0, 1]; one outside it, or not finite, yields
    ``inf``."""
    if out.dtype == torch.bfloat16:
        bound = tol + BF16_ROUNDOFF * (ref.abs() + tol)
    elif out.dtype == torch.float32:
        bound = tol
    else:
        raise TypeError(f"kernel outputs are fp32 or bf16, got {out.dtype}")
    if out.shape != ref.shape:
        raise ValueError(f"shape {tuple(out.shape)} != {tuple(ref.shape)}")
    err = (out.double() - ref).abs()
    ok = err <= bound                # False for NaN
    ratio = torch.where(bound > 0, err / bound, torch.zeros_like(err))
    return torch.where(ok, ratio, torch.full_like(err, float("inf")))


def pack_frag_ref(w: torch.Tensor, G: int, dx: bool = False) -> torch.Tensor:
    """The fragment-packed mirror of ``w [G, N, K]`` (flattened groups
    allowed) by index arithmetic:
    ``P[((g NT + t) KS + ks) 64 + l][j] = W[g][t 16 + (l & 15)]
    [ks 32 + (l >> 4) 8 + j]``, zero out of range; ``dx`` packs W
    transposed.  Returns the flat ``[G * NT * KS * 512]`` tensor."""
    K = w.shape[-1]
    w3 = w.reshape(G, -1, K)
    if dx:
        w3 = w3.transpose(1, 2)
    rows, cols = w3.shape[1], w3.shape[2]
    NT, KS = (rows + 15) // 16, (cols + 31) // 32
    padded = torch.zeros(G, NT * 16, KS * 32, dtype=w.dtype, device=w.device)
    padded[:, :rows, :cols] = w3
    dev = w.device
    lane = torch.arange(64, device=dev)
    r = torch.arange(NT, device=dev)[:, None, None, None] * 16 \
        + (lane & 15)[None, None, :, None]
    c = torch.arange(KS, device=dev)[None, :, None, None] * 32 \
        + ((lane >> 4) * 8)[None, None, :, None] \
        + torch.arange(8, device=dev)[None, None, None, :]
    r, c = torch.broadcast_tensors(r, c)
    return padded[:, r, c].reshape(-1)


def f32_to_bf16_bits(u: torch.Tensor) -> torch.Tensor:
    """The kernels' fp32 -> bf16 conversion on bit patterns (int64 tensors
    holding 32-bit words; returns 16-bit words): round to nearest, ties to
    even — add ``0x7FFF + (bit 16)``, drop the low half.  A NaN must stay a
    NaN; that add would carry one with a small mantissa into Inf or zero.
    Here it gets its quiet bit set and keeps its sign; the kernels use the
    native conversion instruction, which picks its own NaN payload, so only
    the non-NaN words are comparable bit for bit."""
    u = u & 0xFFFFFFFF
    is_nan = (u & 0x7FFFFFFF) > 0x7F800000
    rne = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF
    return torch.where(is_nan, u | 0x00400000, rne) >> 16


# ---------------------------------------------------------------------------
# Squash (K4) and attention-pool (K3) oracles (docs/KERNELS.md "Numerics").
# Float64 references computed from the kernels' exact fp32 / bf16 inputs,
# each returned next to a per-element bound in units of u = 2^-24 (the fp32
# unit roundoff), so a test reports err / bound as for the GEMMs.  The
# bounds' structure follows the kernels' arithmetic; the only allowances
# are those of the transcendental calls, in ulps: four times the worst
# error (rounded up, at least 1) of the fp32 torch call against float64
# over the test inputs (profiles/squash_reference.md) — the device's fast
# variants are not specified that far.  The constants are the kernels'
# fp32 constants widened, not the decimal values.
# ---------------------------------------------------------------------------

SQ_U = 2.0 ** -24
SQ_E_EXP = 4
SQ_E_LOG = 4
SQ_E_TANH = 4
SQ_E_COS = 4
SQ_EPS6 = float(torch.tensor(1e-6, dtype=torch.float32))
SQ_C = float(torch.tensor(0.9189385332046727, dtype=torch.float32))
SQ_EPS_BOUND = 2.0 ** -20       # |e - e64| <= 2^-20 (r + 1)


@torch.no_grad()
def bound_ratio(out: torch.Tensor, ref: torch.Tensor,
                tol: torch.Tensor) -> torch.Tensor:
    """:func:`gemm_bound_ratio` that also accepts a NaN reference: there
    the ratio is 0 if the output is a NaN too and ``inf`` if it is not."""
    nan = torch.isnan(ref)
    z = torch.zeros_like(ref)
    r = gemm_bound_ratio(out, torch.where(nan, z, ref),
                         torch.where(nan, z, tol))
    hit = torch.where(torch.isnan(out.double()), z,
                      torch.full_like(ref, float("inf")))
    return torch.where(nan, hit, r)


@torch.no_grad()
def squash_eps_oracle(ctr, B: int, A: int):
    """``(e, r)`` float64 ``[B, A]``: the Box-Muller draw of k_squash_fwd's
    counter mode.  Element ``idx = i A + a`` hashes
    ``h1 = sm64(c 0x100000001 + 2 idx + 1)``, ``h2 = sm64(h1)``; the
    uniforms ``((h >> 40) + 1) 2^-24`` are exact in float64;
    ``r = sqrt(-2 ln u1)`` and ``e = r cos(2 pi u2)``."""
    if not torch.is_tensor(ctr):
        ctr = torch.tensor(_i64(int(ctr)), dtype=torch.int64)
    c = ctr.reshape(-1)[:1].to(device="cpu", dtype=torch.int64)
    idx = torch.arange(B * A, dtype=torch.int64)
    h1 = _sm64(c * 0x100000001 + idx * 2 + 1)
    h2 = _sm64(h1)
    u1 = (_lsr(h1, 40) + 1).double() * SQ_U
    u2 = (_lsr(h2, 40) + 1).double() * SQ_U
    r = torch.sqrt(-2.0 * torch.log(u1))
    e = r * torch.cos(2.0 * math.pi * u2)
    return e.reshape(B, A), r.reshape(B, A)


@torch.no_grad()
def squash_fwd_oracle(mu: torch.Tensor, lsr: torch.Tensor,
                      eps: torch.Tensor, k: float,
                      t: Optional[torch.Tensor] = None) -> dict:
    """k_squash_fwd in float64 from its fp32 inputs ``mu, lsr, eps [B, A]``
    (any strides).  Returns a dict:

    - ``ls``: fp32, what ``ls_out`` must equal bit for bit —
      ``clamp(lsr, -20, 2)``, a NaN staying a NaN;
    - ``t, tol_t``: ``tanh(mu + exp(ls) eps)`` and
      ``(1 - t^2) du + E_tanh u |t| + 2^-100`` with
      ``du = (E_exp + 2) u |s e| + u |u64|`` (the error of s, the product
      and the sum, carried through tanh's slope);
    - ``logp, tol_logp [B, 1]``: the log-prob computed from the given
      fp32 ``t`` (teacher forcing: the kernel's own saved tanh, so that the
      ill-conditioned ``log(1 - t^2)`` is judged for its own arithmetic
      only) or, without one, from ``t`` above.
      ``tol = (3 A + E_log + 4) u mag + sum_a 2 u / w_a`` with
      ``w = 1 - t^2 + 1e-6f`` and
      ``mag = sum_a (e^2 / 2 + |ls| + C + |ln(k w)|)``; the second term
      carries an absolute error u of ``1 - t t`` (fused or not) and of the
      sum with 1e-6f through the logarithm, and is dropped where
      ``t = +-1``: there ``1 - t t`` is exactly 0 in either order;
    - ``act``: with a given ``t``, fp32 ``float32(k) t`` — one rounded
      product, to be matched bit for bit."""
    A = mu.shape[-1]
    k32 = torch.tensor(float(k), dtype=torch.float32)
    k64 = float(k32)
    ls32 = torch.clamp(lsr.detach().float().cpu(), LOG_STD_MIN, LOG_STD_MAX)
    ls = ls32.double()
    e = eps.detach().cpu().double()
    s = torch.exp(ls)
    u64 = mu.detach().cpu().double() + s * e
    t64 = torch.tanh(u64)
    d_u = (SQ_E_EXP + 2) * SQ_U * (s * e).abs() + SQ_U * u64.abs()
    tol_t = (1.0 - t64 * t64) * d_u + SQ_E_TANH * SQ_U * t64.abs() \
        + GEMM_FLOOR
    out = dict(ls=ls32, t=t64, tol_t=tol_t, act=None)
    if t is not None:
        t32 = t.detach().float().cpu()
        out["act"] = k32 * t32
        tt = t32.double()
    else:
        tt = t64
    w = 1.0 - tt * tt + SQ_EPS6
    lkw = torch.log(k64 * w)
    out["logp"] = (-0.5 * e * e - ls - SQ_C - lkw).sum(-1, keepdim=True)
    mag = (0.5 * e * e + ls.abs() + SQ_C + lkw.abs()).sum(-1, keepdim=True)
    cond = torch.where(tt.abs() == 1.0, torch.zeros_like(w),
                       2.0 * SQ_U / w).sum(-1, keepdim=True)
    out["tol_logp"] = (3 * A + SQ_E_LOG + 4) * SQ_U * mag + cond
    return out


@torch.no_grad()
def squash_bwd_oracle(ga: torch.Tensor, gl: torch.Tensor,
                      lsr: torch.Tensor, ls: torch.Tensor,
                      eps: torch.Tensor, t: torch.Tensor, k: float):
    """``(du, dlsr, tol_du, tol_dlsr)`` float64 ``[B, A]`` of k_squash_bwd
    and k_squash_bwd2 from their fp32 inputs: ``ga [B, A]`` or the twin
    ``[2, B, A]`` (summed), ``gl [B]``, raw ``lsr``, and the forward's
    saved ``ls, eps, t``.

    ``du = T1 + T2``, ``T1 = ga k (1 - t^2)``,
    ``T2 = g 2 t (1 - t^2) / w``, ``w = 1 - t^2 + 1e-6f``;
    ``tol_du = 8 u (|T1| + |T2|) + u (|ga k| + |2 g t| 1e-6f / w^2)`` —
    at most eight roundings on either term, and an absolute error u of
    ``1 - t t`` through both terms' derivatives.
    ``dlsr = m (du e s - g)`` with ``m = 1`` for raw ``lsr`` in [-20, 2],
    0 outside (``tol = 0``: exactly 0) and NaN for a NaN;
    ``tol_dlsr = tol_du |e s| + (E_exp + 4) u (|du e s| + |g|)``."""
    k64 = float(torch.tensor(float(k), dtype=torch.float32))
    ga64 = ga.detach().cpu().double()
    if ga64.dim() == 3:
        ga64 = ga64[0] + ga64[1]
    g = gl.detach().cpu().double().reshape(-1, 1)
    raw = lsr.detach().cpu().double()
    e = eps.detach().cpu().double()
    tt = t.detach().cpu().double()
    s = torch.exp(ls.detach().cpu().double())
    omt2 = 1.0 - tt * tt
    w = omt2 + SQ_EPS6
    T1 = ga64 * k64 * omt2
    T2 = g * 2.0 * tt * omt2 / w
    du = T1 + T2
    tol_du = 8 * SQ_U * (T1.abs() + T2.abs()) + SQ_U * (
        (ga64 * k64).abs() + (2.0 * g * tt).abs() * SQ_EPS6 / (w * w))
    one, zero = torch.ones_like(raw), torch.zeros_like(raw)
    inside = (raw >= LOG_STD_MIN) & (raw <= LOG_STD_MAX)
    m = torch.where(inside, one, torch.where(torch.isnan(raw), raw, zero))
    des = du * e * s
    dlsr = m * (des - g)
    tol_dlsr = torch.where(
        inside,
        tol_du * (e * s).abs() + (SQ_E_EXP + 4) * SQ_U * (des.abs() + g.abs()),
        zero)
    return du, dlsr, tol_du, tol_dlsr


@torch.no_grad()
def attn_pool_oracle(logits: torch.Tensor, z_encs: torch.Tensor,
                     rep: int = 1):
    """``(alpha, tol_alpha [Mz, E], pooled, tol_pooled [M, D])`` float64 of
    k_attn_pool_fwd: ``alpha = softmax(logits [Mz, E])`` and
    ``pooled[r] = sum_e alpha[r % Mz][e] z_encs[e][r]`` with
    ``z_encs [E, M = Mz rep, D]``.  ``tol_alpha = (E + E_exp + 4) u alpha``
    (the difference to the maximum, the exponential, E additions, the
    reciprocal and the product); the pooled value is a GEMM of n = E terms
    with ``mag = sum_e alpha_e |z_e|`` plus alpha's own error on ``mag``.
    The output is bf16: use :func:`bound_ratio`."""
    E = logits.shape[-1]
    alpha = torch.softmax(logits.detach().cpu().double(), -1)
    c_alpha = (E + SQ_E_EXP + 4) * SQ_U
    tol_alpha = c_alpha * alpha + GEMM_FLOOR
    z = z_encs.detach().cpu().double()
    al = alpha.repeat(rep, 1)                     # row r -> alpha[r % Mz]
    pooled = torch.einsum("me,emd->md", al, z)
    mag = torch.einsum("me,emd->md", al, z.abs())
    tol = (E + 2) * GEMM_ULP * mag + c_alpha * mag + GEMM_FLOOR
    return alpha, tol_alpha, pooled, tol


@torch.no_grad()
def attn_pool_bwd_oracle(z_encs: torch.Tensor, alpha: torch.Tensor,
                         dz: torch.Tensor):
    """k_attn_pool_bwd from ``z_encs [E, M, D]`` fp32, ``alpha [M, E]`` fp32
    and the bf16 ``dz [M, D]`` (the columns the kernel reads).  Returns
    ``(dzencs_bits, dlogits, tol)``: the 16-bit words of
    ``bf16_rne(float32(alpha_e dz))`` as int64 ``[E, M, D]`` — one rounded
    product and one cast, to be matched bit for bit — and float64
    ``dlogits = alpha_e (s_e - t)``, ``s_e = sum_d z_e dz``,
    ``t = sum_e alpha_e s_e``, a GEMM of ``n = D + E + 4`` terms with
    ``mag = alpha_e (sum_d |z_e dz| + sum_e' alpha_e' sum_d |z_e' dz|)``
    (bf16 output)."""
    E, M, D = z_encs.shape
    a32 = alpha.detach().float().cpu()
    dz32 = dz.detach().float().cpu()
    prod = a32.t().unsqueeze(-1) * dz32.unsqueeze(0)          # fp32, RN
    bits = f32_to_bf16_bits(prod.contiguous().view(torch.int32).long())
    z, a, d = z_encs.detach().cpu().double(), a32.double(), dz32.double()
    s = torch.einsum("emd,md->me", z, d)
    sabs = torch.einsum("emd,md->me", z.abs(), d.abs())
    t = (a * s).sum(-1, keepdim=True)
    tabs = (a * sabs).sum(-1, keepdim=True)
    dlogits = a * (s - t)
    mag = a * (sabs + tabs)
    tol = (D + E + 4 + 2) * GEMM_ULP * mag + GEMM_FLOOR
    return bits, dlogits, tol


# ---------------------------------------------------------------------------
# TD-target and loss oracles (K5-K7; docs/KERNELS.md "Numerics").  Float64
# references of k_td_target(_mt), k_critic_loss_*, k_actor_alpha_loss_* and
# the two fused-tail kernels, each next to a bound in units of u = 2^-24
# derived from the kernels' operation sequence.  Elementwise outputs get one
# rounding per operation on its own magnitude plus the propagated input
# error; a sum S of fp32 terms gets
#     |S - S64| <= sum |dterm_i| + (L + 2) u sum |term_i|,
# L the longest chain of dependent additions (:func:`loss_chain`).  The one
# allowance that is no plain rounding is __expf, v_exp_f32(x log2e) on
# gfx950: relative E_fexp(x) u = (LOSS_E_FEXP + 2 |x|) u, the product's
# rounding scaled by |x| plus the instruction's error.  The constant part
# started at 4 (a 1-ulp instruction, 2 u, doubled); measured on the device
# over the tests' log_alpha the worst error is 3.945 u, more than a quarter
# of that allowance, so it is four times the worst observed, rounded up:
# 16 (profiles/loss_reference.md).  Constants are the
# kernels' fp32 constants widened.  Backward coefficients are judged from
# the wsum the kernel was handed, sums from the y they were given.
# ---------------------------------------------------------------------------

LOSS_CE = float(torch.tensor(1.4189385332046727, dtype=torch.float32))
LOSS_E_FEXP = 16.0


def _f32(v) -> float:
    return float(torch.tensor(float(v), dtype=torch.float32))


def _vec64(x: torch.Tensor) -> torch.Tensor:
    return x.detach().cpu().double().reshape(-1)


def loss_e_fexp(x: torch.Tensor) -> torch.Tensor:
    """Relative error bound of the kernels' ``__expf(x)``."""
    return (LOSS_E_FEXP + 2.0 * x.abs()) * SQ_U


def loss_task_index(states: torch.Tensor, T: int) -> torch.Tensor:
    """Task of every row, int64 ``[B]``: the position of the FIRST maximum
    of the last ``T`` columns (an all-zero row is task 0); 0 for T == 1."""
    st = states.detach().cpu()
    B = st.shape[0]
    if T <= 1:
        return torch.zeros(B, dtype=torch.int64)
    suf = st[:, st.shape[1] - T:]
    mx = suf.max(-1, keepdim=True).values
    pos = torch.arange(T).expand(B, T)
    return torch.where(suf == mx, pos, torch.full_like(pos, T)).min(-1).values


def loss_chain(B: int, kind: str, nblk: int = 1) -> int:
    """Longest chain of dependent fp32 additions of a reduction over B
    rows.  ``mb`` (k_*_loss_fwd_mb and the fused kernels, nblk blocks):
    per-thread strided adds, 6 butterfly steps, 3 adds of the four wave
    partials, nblk slots.  ``1wg``: the same in one block, no slots.
    ``agb`` (alpha_grad_block): per-thread adds, 2 for the four LDS
    columns, 6 butterfly steps.  ``ws`` (per-block task sums of
    k_actor_alpha_loss_bwd2 / the fused kernel): 2 + 6 + nblk slots."""
    if kind == "mb":
        return -(-B // (256 * nblk)) + 6 + 3 + nblk
    if kind == "1wg":
        return -(-B // 256) + 6 + 3
    if kind == "agb":
        return -(-B // 256) + 2 + 6
    if kind == "ws":
        return 2 + 6 + nblk
    raise ValueError(kind)


def loss_alpha(log_alpha: torch.Tensor, T: int):
    """``(alpha, e_alpha) [T]``: float64 ``exp(log_alpha)`` and the relative
    error bound of the kernels' ``__expf``."""
    la = _vec64(log_alpha)[:T]
    return torch.exp(la), loss_e_fexp(la)


def loss_task_weights(log_alpha: torch.Tensor, T: int):
    """``(w, e_w) [T]``: float64 ``softmax(-exp(log_alpha))`` and the
    relative error bound of fill_task_weights.  With ``a = exp(la)`` (error
    ``a e_a``) and ``m = min a`` the exponent ``z = m - a`` carries
    ``dz = u |z| + a e_a + m e_m``, so a numerator is off by
    ``rho = E_fexp(z) u + dz``; the denominator by ``max rho`` plus T - 1
    additions; one more rounding for the division."""
    a, e_a = loss_alpha(log_alpha, T)
    k = int(torch.argmin(a))
    z = a[k] - a
    dz = SQ_U * z.abs() + a * e_a + a[k] * e_a[k]
    rho = loss_e_fexp(z) + dz
    ex = torch.exp(z)
    return ex / ex.sum(), rho + rho.max() + (T + 1) * SQ_U


def loss_sum(term: torch.Tensor, dterm: torch.Tensor, L: int):
    """``(S, tol)`` of an fp32 sum whose longest addition chain is L."""
    return term.sum(), dterm.sum() + (L + 2) * SQ_U * term.abs().sum() \
        + GEMM_FLOOR


@torch.no_grad()
def td_target_oracle(r, d, q1, q2, lp, gamma: float, rs: float,
                     alpha: Optional[torch.Tensor] = None,
                     states: Optional[torch.Tensor] = None,
                     log_alpha: Optional[torch.Tensor] = None, T: int = 1):
    """``(y, tol)`` float64 ``[B]``:
    ``y = rs r + gamma (1 - d) (min(q1, q2) - alpha lp)``, a NaN in either
    Q staying one.  With ``states, log_alpha, T`` it is k_td_target_mt /
    td_target_value: ``alpha = exp(log_alpha[task])`` carries
    ``dalpha = alpha E_fexp u`` and ``x = fma(-alpha, lp, qmin)`` one
    rounding, ``dx = u |x| + dalpha |lp|``.  With a per-sample ``alpha`` it
    is k_td_target, whose contraction is the compiler's: the product
    ``alpha lp`` may round on its own (``+ u |alpha lp|``), and every other
    fusion only removes a rounding.  Then ``g = gamma (1 - d)`` (``1 - d``
    exact for d in {0, 1}), ``p = g x``, ``q = rs r``, ``y = q + p``:
    ``tol = u (|q| + 2 |p| + |y|) + |g| dx (+ u gamma |1 - d| |x|)``."""
    r, d, q1, q2, lp = (_vec64(v) for v in (r, d, q1, q2, lp))
    if alpha is not None:
        a = _vec64(alpha)
        da = torch.zeros_like(a)
    else:
        t = loss_task_index(states, T)
        a_t, e_t = loss_alpha(log_alpha, T)
        a, da = a_t[t], (a_t * e_t)[t]
    g32, s32 = _f32(gamma), _f32(rs)
    x = torch.minimum(q1, q2) - a * lp
    dx = SQ_U * x.abs() + da * lp.abs()
    if alpha is not None:
        dx = dx + SQ_U * (a * lp).abs()
    omd = 1.0 - d
    d_omd = torch.where((d == 0) | (d == 1), torch.zeros_like(d),
                        SQ_U * omd.abs())
    g = g32 * omd
    p, q = g * x, s32 * r
    y = q + p
    tol = SQ_U * (q.abs() + 2.0 * p.abs() + y.abs()) + g.abs() * dx \
        + g32 * d_omd * x.abs() + GEMM_FLOOR
    return y, tol


def _loss_rows(states, log_alpha, T: int, use_w: int, B: int):
    """Per-row task, weight and the weight's relative error."""
    t = loss_task_index(states, T)
    if use_w:
        w_t, e_t = loss_task_weights(log_alpha, T)
        return t, w_t[t], e_t[t]
    return t, torch.ones(B, dtype=torch.float64), \
        torch.zeros(B, dtype=torch.float64)


@torch.no_grad()
def critic_loss_oracle(q1, q2, y, states, log_alpha, T: int, use_w: int,
                       L: int, wsum: Optional[float] = None,
                       gscale=None) -> dict:
    """The critic loss kernels in float64 from the fp32 ``q1, q2, y [B]``
    they are given.  ``out, tol_out [7]``: ``r0 = sum w (y - q1)^2``,
    ``r1`` likewise, ``r2 = sum w`` at 3, 4, 5 (a term is off by
    ``(4 u + e_w) |term|``: the difference twice, two products, the
    weight); ``out[2] = r2`` or exactly 1 without weights;
    ``out[0, 1] = r / (out[2] B)`` and ``out[6] = (r0 + r1) / (out[2] B)``
    add r2's relative error and the roundings of the product, the division
    (and the sum).  With ``wsum`` — the fp32 value the backward was
    handed — also ``dq, tol_dq [2, B]``:
    ``dq = g (w / wsum / B) (-2) (y - q)``, relative
    ``e_w + 4 u`` (``+ u`` with a ``gscale``, ``- u`` without weights)."""
    q1, q2, y = (_vec64(v) for v in (q1, q2, y))
    B = q1.numel()
    _, w, ew = _loss_rows(states, log_alpha, T, use_w, B)
    d1, d2 = y - q1, y - q2
    t1, t2 = w * d1 * d1, w * d2 * d2
    rel = 4 * SQ_U + ew
    S0, tol0 = loss_sum(t1, rel * t1.abs(), L)
    S1, tol1 = loss_sum(t2, rel * t2.abs(), L)
    Sw, tolw = loss_sum(w, ew * w, L)
    one, zero = torch.tensor(1.0, dtype=torch.float64), \
        torch.tensor(0.0, dtype=torch.float64)
    ws, tws = (Sw, tolw) if use_w else (one, zero)
    rel_w = tws / ws
    den = ws * B
    o0, o1, o6 = S0 / den, S1 / den, (S0 + S1) / den
    res = dict(
        out=torch.stack([o0, o1, ws, S0, S1, Sw, o6]),
        tol_out=torch.stack([
            tol0 / den + o0.abs() * (rel_w + 2 * SQ_U),
            tol1 / den + o1.abs() * (rel_w + 2 * SQ_U),
            tws, tol0, tol1, tolw,
            (tol0 + tol1) / den + o6.abs() * (rel_w + 3 * SQ_U)]))
    if wsum is not None:
        c = (w / float(wsum) if use_w else w) / B
        relc = ew + (4 if use_w else 3) * SQ_U
        g = [1.0, 1.0]
        if gscale is not None:
            g = [_f32(v) for v in torch.as_tensor(gscale).reshape(-1).tolist()]
            relc = relc + SQ_U
        dq = torch.stack([g[0] * c * -2.0 * d1, g[1] * c * -2.0 * d2])
        res.update(dq=dq, tol_dq=dq.abs() * relc + GEMM_FLOOR)
    return res


@torch.no_grad()
def actor_alpha_loss_oracle(aq1, aq2, lp, ls, states, log_alpha, T: int,
                            use_w: int, H_bar: float, L: int,
                            wsum: Optional[float] = None, gscale=None,
                            L_dla: Optional[int] = None,
                            dla_n: Optional[int] = None) -> dict:
    """The actor / alpha loss kernels in float64 from their fp32 inputs.

    ``out, tol_out [8]``: the raw sums at 4..7 —
    ``s_pl = sum -w (min(aq1, aq2) - alpha lp)`` (a NaN Q staying one; a
    term is off by ``w (u |alpha lp| + dalpha |lp| + u |x|) + (u + e_w)
    |term|``), ``s_w = sum w``, ``s_al = sum la (lp + H)`` (``2 u |term|``),
    ``s_en = sum (CE A + sum_a ls)`` (one rounding per partial sum) — and
    ``out[0] = s_pl / (out[1] B)``, ``out[1] = s_w`` or exactly 1,
    ``out[2] = -s_al / B``, ``out[3] = s_en / B``.  The bounds of the
    signed sums are on ``sum |term|``.

    With ``wsum`` (the fp32 value the backward used) the backward:
    ``c = w / wsum / B``; ``daq [2, B]`` holds ``-g c`` in the twin with the
    smaller Q (the first on a tie, the second beside a NaN) and an exact 0
    in the other; ``dlp = g c alpha``.  Without weights and ``gscale``,
    ``daq_bits`` is the 16-bit word of ``bf16_rne(float32(-1 / B))``, to be
    matched bit for bit.  With ``L_dla`` the alpha gradient ``dla [dla_n]``:
    ``sum_{i in t} gal (-(lp + H)) / B`` per task (two roundings a term,
    three with a ``gscale``), exactly 0 for a task without rows and past
    T."""
    aq1, aq2, lp = (_vec64(v) for v in (aq1, aq2, lp))
    ls = ls.detach().cpu().double()
    B, A = aq1.numel(), ls.shape[1]
    t, w, ew = _loss_rows(states, log_alpha, T, use_w, B)
    a_t, e_t = loss_alpha(log_alpha, T)
    la = _vec64(log_alpha)[:T][t]
    al, e_al = a_t[t], e_t[t]
    H = _f32(H_bar)
    x = torch.minimum(aq1, aq2) - al * lp
    dx = SQ_U * (al * lp).abs() + al * e_al * lp.abs() + SQ_U * x.abs()
    t_pl = -w * x
    S0, tol0 = loss_sum(t_pl, w * dx + t_pl.abs() * (SQ_U + ew), L)
    Sw, tolw = loss_sum(w, ew * w, L)
    t_al = la * (lp + H)
    S2, tol2 = loss_sum(t_al, 2 * SQ_U * t_al.abs(), L)
    part = torch.cumsum(
        torch.cat([torch.full((B, 1), LOSS_CE * A, dtype=torch.float64),
                   ls.reshape(B, A)], 1), 1)
    S3, tol3 = loss_sum(part[:, -1], SQ_U * part.abs().sum(1), L)
    one, zero = torch.tensor(1.0, dtype=torch.float64), \
        torch.tensor(0.0, dtype=torch.float64)
    ws, tws = (Sw, tolw) if use_w else (one, zero)
    den = ws * B
    o0, o2, o3 = S0 / den, -S2 / B, S3 / B
    res = dict(
        out=torch.stack([o0, ws, o2, o3, S0, Sw, S2, S3]),
        tol_out=torch.stack([
            tol0 / den + o0.abs() * (tws / ws + 2 * SQ_U), tws,
            tol2 / B + SQ_U * o2.abs(), tol3 / B + SQ_U * o3.abs(),
            tol0, tolw, tol2, tol3]))
    g = [1.0, 1.0]
    rg = 0.0
    if gscale is not None:
        g = [_f32(v) for v in torch.as_tensor(gscale).reshape(-1).tolist()]
        rg = SQ_U
    if wsum is not None:
        c = (w / float(wsum) if use_w else w) / B
        relc = (ew + 2 * SQ_U if use_w else SQ_U) + rg
        first = aq1 <= aq2
        v = -g[0] * c
        z = torch.zeros_like(v)
        daq = torch.stack([torch.where(first, v, z), torch.where(first, z, v)])
        dlp = g[0] * c * al
        res.update(daq=daq, tol_daq=daq.abs() * relc, dlp=dlp,
                   tol_dlp=dlp.abs() * (relc + SQ_U + e_al) + GEMM_FLOOR)
        if not use_w and gscale is None:
            c32 = -(torch.tensor(1.0) / torch.tensor(float(B)))
            bits = f32_to_bf16_bits(c32.view(torch.int32).long())
            zb = torch.zeros(B, dtype=torch.int64)
            res["daq_bits"] = torch.stack([torch.where(first, bits, zb),
                                           torch.where(first, zb, bits)])
    if L_dla is not None:
        n = T if dla_n is None else dla_n
        term = g[1] * -(lp + H) / B
        nr = 3 if gscale is not None else 2
        dla = torch.zeros(n, dtype=torch.float64).index_add_(0, t, term)
        mag = torch.zeros(n, dtype=torch.float64).index_add_(0, t, term.abs())
        res.update(dla=dla, tol_dla=(nr + L_dla + 2) * SQ_U * mag)
    return res
