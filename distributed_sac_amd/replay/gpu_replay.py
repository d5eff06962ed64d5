"""Device-resident sharded replay buffer.

MI355X-first re-design of the reference's replay layer
(LunarLander_Distributed_SAC/src/replay_buffer.py:13-77 single deque;
MT10_Distributed_MTSAC/src/replay_buffers.py:13-107 per-task deques):

- Transitions live as SoA ring buffers in device memory.  The reference's
  1e6-transition MT10 buffer is ~250 MB fp32 — trivial against 288 GB HBM3E
  per GPU, so the whole buffer is GPU-resident and a minibatch sample is a
  device-side gather with NO host round-trip (replaces SURVEY §2.6 K12:
  np.vstack + torch.from_numpy().to(device) per update).
- Ingest crosses the PCIe/host boundary once, batched: numpy transition
  blocks are staged into a reusable pinned buffer and copied with one
  async H2D per field (overlappable with the update stream).  Ring blocks
  can instead take the packed path (``stage_packed`` / ``commit_packed``
  / ``flush_packed``): a whole drain is packed into one pinned staging
  buffer, copied H2D once on a copy stream and scattered into the shards
  by one ``k_replay_ingest`` launch on the main stream.
- MT variants shard per task with stratified sampling (batch//num_tasks
  from each shard, shuffled concat) and ``len = min over shards`` —
  reference replay_buffers.py:37-41,67-100 semantics.

Deviation from the reference, by default: minibatch indices are drawn with
replacement (``floor(u * size)`` in ``k_replay_sample``, ``torch.randint``
on the host path) where the reference's ``random.sample`` draws without —
while a shard holds a few thousand entries, up to ~15% of a 1280 batch's
rows collide (docs/PARITY.md).  ``sampling="without_replacement"`` (or
``DSAC_SAMPLING=without_replacement``) restores the reference's
semantics: each shard's rows of one batch are distinct, drawn by a keyed
permutation evaluated per row (``k_replay_sample_norepl`` /
``torch_ref.replay_sample_indices_norepl``) — inside the captured update,
with no host round trip and no 1e6-element randperm.

``sampling="prioritized"`` (net-new; the reference has none) is proportional
prioritized experience replay with importance-sampling weights: priorities
live next to the rings as a flat two-level sum, the draw, the weights and the
priority write-back all run inside the captured update (docs/KERNELS.md
"Prioritized replay").
"""

from __future__ import annotations

import os
from typing import Dict, List, Optional

import numpy as np
import torch

FIELDS = ("states", "actions", "rewards", "next_states", "dones")
SAMPLING_MODES = ("replace", "without_replacement", "prioritized")
PER_DEFAULTS = {"per_alpha": 0.6, "per_beta": 0.4,
                "per_beta_anneal_steps": 0, "per_eps": 1e-6}


def check_per_params(per_alpha=None, per_beta=None,
                     per_beta_anneal_steps=None, per_eps=None) -> dict:
    """The four prioritized-replay settings with defaults filled in;
    ``ValueError`` for a value outside its range."""
    out = dict(PER_DEFAULTS)
    given = {"per_alpha": per_alpha, "per_beta": per_beta,
             "per_beta_anneal_steps": per_beta_anneal_steps,
             "per_eps": per_eps}
    for k, v in given.items():
        if v is None:
            continue
        try:
            out[k] = int(v) if k == "per_beta_anneal_steps" else float(v)
            exact = out[k] == v
        except (TypeError, ValueError):
            exact = False
        if not exact or isinstance(v, bool):
            raise ValueError(f"{k} must be a number, got {v!r}")
    if not 0.0 <= out["per_alpha"] < float("inf"):
        raise ValueError(f"per_alpha must be >= 0, got {per_alpha!r}")
    if not 0.0 <= out["per_beta"] <= 1.0:
        raise ValueError(f"per_beta must be in [0, 1], got {per_beta!r}")
    if out["per_beta_anneal_steps"] < 0:
        raise ValueError("per_beta_anneal_steps must be >= 0, got "
                         f"{per_beta_anneal_steps!r}")
    if not 0.0 < out["per_eps"] < float("inf"):
        raise ValueError(f"per_eps must be > 0, got {per_eps!r}")
    return out


class ReplayShard:
    """One SoA ring buffer (one task shard).

    Field tensors may be externally provided views (ShardedReplay stacks all
    shards as [T, cap, D] so the fused sampling kernel gathers across tasks
    in one launch).
    """

    def __init__(self, capacity: int, state_dim: int, action_dim: int,
                 device: torch.device | str = "cpu", buffers=None,
                 size_dev: Optional[torch.Tensor] = None):
        self.capacity = int(capacity)
        self.device = torch.device(device)
        self.state_dim = state_dim
        self.action_dim = action_dim
        dev = self.device
        if buffers is not None:
            (self.states, self.actions, self.rewards, self.next_states,
             self.dones) = buffers
        else:
            self.states = torch.zeros(self.capacity, state_dim, device=dev)
            self.actions = torch.zeros(self.capacity, action_dim, device=dev)
            self.rewards = torch.zeros(self.capacity, 1, device=dev)
            self.next_states = torch.zeros(self.capacity, state_dim, device=dev)
            self.dones = torch.zeros(self.capacity, 1, device=dev)
        self.write_ptr = 0
        self.size = 0
        # device-resident size for hipGraph-safe sampling (updated by
        # append OUTSIDE any captured region; read inside the graph)
        self.size_dev = (size_dev if size_dev is not None
                         else torch.zeros(1, device=dev))
        # prioritized replay: called with (first row, rows) after a write
        self.on_append = None

    def __len__(self) -> int:
        return self.size

    @torch.no_grad()
    def append(self, states: torch.Tensor, actions: torch.Tensor,
               rewards: torch.Tensor, next_states: torch.Tensor,
               dones: torch.Tensor) -> None:
        """Append a block of n transitions (device tensors), wrapping."""
        n = states.shape[0]
        if n == 0:
            return
        if n >= self.capacity:  # keep only the newest `capacity`
            states, actions = states[-self.capacity:], actions[-self.capacity:]
            rewards = rewards[-self.capacity:]
            next_states, dones = next_states[-self.capacity:], dones[-self.capacity:]
            n = self.capacity
        # blocks are contiguous, so ingestion is plain slice copies —
        # straight (async DMA) H2D when the source is pinned host memory,
        # no arange/index_copy kernels.  Sources may be host OR device.
        pairs = ((self.states, states), (self.actions, actions),
                 (self.rewards, rewards.reshape(n, 1)),
                 (self.next_states, next_states),
                 (self.dones, dones.reshape(n, 1)))
        wp = self.write_ptr
        head = min(n, self.capacity - wp)
        for dst, src in pairs:
            dst[wp:wp + head].copy_(src[:head], non_blocking=True)
            if head < n:   # wrap: the tail goes to the front
                dst[: n - head].copy_(src[head:], non_blocking=True)
        self.write_ptr = (wp + n) % self.capacity
        if self.on_append is not None:
            self.on_append(wp, n)
        new_size = min(self.size + n, self.capacity)
        if new_size != self.size:   # no kernel once the shard is full
            self.size = new_size
            self.size_dev.fill_(float(new_size))

    @torch.no_grad()
    def sample_indices(self, n: int,
                       generator: Optional[torch.Generator] = None,
                       graph_safe: bool = False) -> torch.Tensor:
        if graph_safe:
            # hipGraph-capturable draw: default-generator rand (philox with
            # graph-managed offsets) scaled by the device-resident size.
            # rand < 1.0 strictly and sizes < 2^24, so floor(r*size) < size.
            r = torch.rand(n, device=self.device)
            return (r * self.size_dev).long()
        return torch.randint(0, self.size, (n,), device=self.device,
                             generator=generator)

    @torch.no_grad()
    def gather(self, idx: torch.Tensor) -> Dict[str, torch.Tensor]:
        return {
            "states": self.states.index_select(0, idx),
            "actions": self.actions.index_select(0, idx),
            "rewards": self.rewards.index_select(0, idx),
            "next_states": self.next_states.index_select(0, idx),
            "dones": self.dones.index_select(0, idx),
        }

    @torch.no_grad()
    def sample(self, n: int, generator: Optional[torch.Generator] = None,
               graph_safe: bool = False):
        return self.gather(self.sample_indices(n, generator, graph_safe))


class _StagingPair:
    """One host (pinned on GPU) + device staging buffer of the packed
    ingest path.  On CPU both names refer to the same tensor."""

    def __init__(self, floats: int, device: torch.device):
        cuda = device.type == "cuda"
        self.host = torch.zeros(floats, pin_memory=cuda)
        self.host_i32 = self.host.view(torch.int32)
        self.dev = torch.empty(floats, device=device) if cuda else self.host
        self.copy_event = torch.cuda.Event() if cuda else None
        self.done_event = torch.cuda.Event() if cuda else None
        self.free = True          # False from stage until its scatter is done
        self.scattered = False    # scatter launched, done_event recorded


class _PackedBatch:
    """Host-side bookkeeping of one packed batch being built/in flight."""

    def __init__(self, pair: _StagingPair, off: int, num_tasks: int,
                 wp0: List[int], size0: List[int]):
        self.pair = pair
        self.off = off            # float cursor: end of the staged payloads
        self.desc: List[int] = []
        self.n_desc = 0
        self.rows = 0
        self.rows_t = [0] * num_tasks
        self.wp0, self.size0 = wp0, size0   # restored if the build aborts
        self.post_wp: List[int] = []
        self.post_size: List[int] = []
        self.used = 0


class ShardedReplay:
    """Per-task shards + stratified sampling (MT semantics) with a pinned
    staging path for host-produced transitions.

    With ``num_tasks == 1`` this is the single-buffer LL/VSAC replay.
    """

    def __init__(self, buffer_size: int, num_tasks: int, state_dim: int,
                 action_dim: int, device: torch.device | str = "cpu",
                 seed: Optional[int] = None,
                 sampling: Optional[str] = None,
                 per_alpha: Optional[float] = None,
                 per_beta: Optional[float] = None,
                 per_beta_anneal_steps: Optional[int] = None,
                 per_eps: Optional[float] = None):
        # "replace" (default): independent uniform draws per row;
        # "without_replacement": each shard's rows of a batch are distinct
        # (the reference's random.sample), drawn by a keyed permutation;
        # "prioritized": proportional to per-row priorities, with
        # importance-sampling weights (the per_* settings)
        if sampling is None:
            sampling = os.environ.get("DSAC_SAMPLING", "replace")
        if sampling not in SAMPLING_MODES:
            raise ValueError(f"sampling must be 'replace', "
                             f"'without_replacement' or 'prioritized', "
                             f"got {sampling!r}")
        self.sampling = sampling
        per = check_per_params(per_alpha, per_beta, per_beta_anneal_steps,
                               per_eps)
        self.per_alpha, self.per_eps = per["per_alpha"], per["per_eps"]
        self.per_beta0 = per["per_beta"]
        self.per_beta_anneal_steps = per["per_beta_anneal_steps"]
        self.num_tasks = num_tasks
        self.device = torch.device(device)
        per_task = int(buffer_size) // num_tasks  # reference replay_buffers.py:37-41
        dev = self.device
        # stacked [T, cap, D] field storage; shards are views into it so the
        # fused k_replay_sample kernel gathers the whole stratified batch in
        # one launch.
        self.f_states = torch.zeros(num_tasks, per_task, state_dim, device=dev)
        self.f_actions = torch.zeros(num_tasks, per_task, action_dim, device=dev)
        self.f_rewards = torch.zeros(num_tasks, per_task, 1, device=dev)
        self.f_next_states = torch.zeros(num_tasks, per_task, state_dim,
                                         device=dev)
        self.f_dones = torch.zeros(num_tasks, per_task, 1, device=dev)
        self.sizes_dev = torch.zeros(num_tasks, device=dev)
        self.shards: List[ReplayShard] = [
            ReplayShard(per_task, state_dim, action_dim, device,
                        buffers=(self.f_states[t], self.f_actions[t],
                                 self.f_rewards[t], self.f_next_states[t],
                                 self.f_dones[t]),
                        size_dev=self.sizes_dev[t:t + 1])
            for t in range(num_tasks)]
        # prioritized replay state (this mode only): leaves, block sums
        # over PER_BLOCK leaves, per-shard total and running maximum, beta
        self.per_prio = self.per_bsum = self.per_total = None
        self.per_max = self.per_beta = self._per_ws = None
        if sampling == "prioritized":
            from ..ops import torch_ref
            if per_task < 1 or per_task > (1 << 24):
                raise ValueError("prioritized replay: shard capacity must be "
                                 "in [1, 2^24]")
            nb = (per_task + torch_ref.PER_BLOCK - 1) // torch_ref.PER_BLOCK
            self.per_prio = torch.zeros(num_tasks, per_task, device=dev)
            self.per_bsum = torch.zeros(num_tasks, nb, device=dev)
            self.per_total = torch.zeros(num_tasks, device=dev)
            self.per_max = torch.ones(num_tasks, device=dev)
            self.per_beta = torch.full((1,), self.per_beta0, device=dev)
            self._per_ws = torch.zeros(2, dtype=torch.int32, device=dev)
            for t, shard in enumerate(self.shards):
                shard.on_append = (
                    lambda start, n, t=t: self._per_ingest(t, start, n))
        self.generator = None
        if seed is not None:
            self.generator = torch.Generator(device=self.device)
            self.generator.manual_seed(seed)
        self._rng_ctr = None     # optional int64 counter (attach_rng)
        self._empty_rnd = None
        # packed ingest (stage_packed / commit_packed / flush_packed):
        # staging pairs are allocated at first use
        self._pk_pairs: List[_StagingPair] = []
        self._pk_pending: List[_PackedBatch] = []   # staged, not committed
        self._pk_copy_stream = None
        self._pk_max_desc = 0
        self.packed_batches = 0   # batches committed so far
        self._pk_hdr_words = 0
        self._pk_open_batch: Optional[_PackedBatch] = None
        # write pointers / sizes as of the last STAGED batch; the shards'
        # own write_ptr/size follow at commit
        self._pk_wp = [0] * num_tasks
        self._pk_size = [0] * num_tasks

    def attach_rng(self, ctr: torch.Tensor) -> None:
        """Use the engine's counter-based device RNG for graph-safe
        index draws (the counter is bumped once per update by the fused
        Adam prolog kernel)."""
        self._rng_ctr = ctr

    # -- prioritized replay ----------------------------------------------
    def _per_native(self):
        """The extension if the priority kernels run (GPU, native on)."""
        if self.device.type == "cuda":
            from ..ops import native, native_enabled
            if native_enabled():
                return native()
        return None

    def _per_state(self):
        return (self.per_prio, self.per_bsum, self.per_total, self.per_max)

    def _per_ingest(self, t: int, start: int, rows: int) -> None:
        """Rows ``[start, start + rows) mod cap`` of shard t were written:
        they receive the shard's running maximum priority (read on the
        device, never on the host)."""
        ext = self._per_native()
        if ext is not None:
            ext.per_ingest_range(*self._per_state(), self._per_ws, t,
                                 int(start), int(rows))
        else:
            from ..ops import torch_ref
            torch_ref.per_ingest_(*self._per_state(), t, start, rows)

    def set_per_beta(self, beta: float) -> None:
        """Change the importance-sampling exponent; the sampling kernel
        reads it from device memory, so a captured update follows."""
        if self.per_beta is None:
            raise RuntimeError("set_per_beta needs sampling='prioritized'")
        if not 0.0 <= float(beta) <= 1.0:
            raise ValueError(f"per_beta must be in [0, 1], got {beta!r}")
        self.per_beta.fill_(float(beta))

    def anneal_per_beta(self, grad_steps: int) -> float:
        """Linear anneal from ``per_beta`` to 1.0 over
        ``per_beta_anneal_steps`` gradient steps (0: constant)."""
        beta = self.per_beta0
        if self.per_beta_anneal_steps > 0:
            f = min(1.0, max(0.0, grad_steps / self.per_beta_anneal_steps))
            beta = self.per_beta0 + f * (1.0 - self.per_beta0)
        self.set_per_beta(beta)
        return beta

    @torch.no_grad()
    def update_priorities(self, indices: torch.Tensor,
                          new_priorities: torch.Tensor,
                          _zeroed: bool = False) -> None:
        """Write new priorities back: ``indices`` are the flat row indices
        a prioritized ``sample()`` returned, ``new_priorities`` one value
        each.  A row listed more than once keeps the maximum of its values;
        the shard's running maximum is raised; block sums and totals are
        re-summed.  Capturable (no host round trip on the GPU path)."""
        if self.per_prio is None:
            raise RuntimeError("update_priorities needs "
                               "sampling='prioritized'")
        idx = indices.reshape(-1)
        newp = new_priorities.reshape(-1)
        if idx.numel() != newp.numel():
            raise ValueError("one new priority per index")
        ext = self._per_native()
        if ext is None:
            from ..ops import torch_ref
            torch_ref.per_update_(*self._per_state(), idx, newp)
            return
        for o in range(0, idx.numel(), 8192):
            ext.per_update(*self._per_state(), idx[o:o + 8192].contiguous(),
                           newp[o:o + 8192].float().contiguous(),
                           self._per_ws, _zeroed)
    def __len__(self) -> int:
        """min over shards (reference replay_buffers.__len__:102-107)."""
        return min(len(s) for s in self.shards)

    @property
    def total_size(self) -> int:
        return sum(len(s) for s in self.shards)

    def _stage(self, name: str, arr: np.ndarray) -> torch.Tensor:
        """numpy -> pinned host tensor -> async device copy.

        Uses torch's caching host allocator (``pin_memory()``): it records
        the H2D copy's event and defers buffer reuse until it completes —
        a hand-cached pinned buffer here would let the NEXT append's host
        write race an in-flight copy."""
        t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32))
        if self.device.type == "cuda":
            return t.pin_memory().to(self.device, non_blocking=True)
        return t

    # -- packed ingest ---------------------------------------------------
    # One H2D copy + one scatter launch per batch of blocks (format:
    # docs/KERNELS.md "packed replay batch").  stage_packed() packs blocks
    # into a free staging pair and starts its copy on a dedicated stream;
    # commit_packed() launches the scatter ON THE CURRENT (main) STREAM for
    # batches whose copy already finished, so the main stream never waits
    # for PCIe and the scatter is ordered against the sampler like the
    # per-block slice copies.  Host-visible size/write_ptr/len() change at
    # commit.  append/append_numpy/sample flush pending batches first.

    @property
    def _row_floats(self) -> int:
        return 2 * self.f_states.shape[2] + self.f_actions.shape[2] + 2

    def configure_packed(self, payload_floats: int, max_desc: int = 256,
                         pairs: int = 4) -> None:
        """(Re)allocate the staging pairs: ``pairs`` (>= 2) buffers holding
        up to ``max_desc`` blocks / ``payload_floats`` payload floats per
        batch.  Called with defaults at first use; flushes first."""
        from ..ops import torch_ref
        self.flush_packed()
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)  # no scatter reads old pairs
            if self._pk_copy_stream is None:
                self._pk_copy_stream = torch.cuda.Stream(self.device)
        self._pk_max_desc = int(max_desc)
        self._pk_hdr_words = torch_ref.packed_header_words(
            self.num_tasks, self._pk_max_desc)
        floats = self._pk_hdr_words + int(payload_floats)
        self._pk_pairs = [_StagingPair(floats, self.device)
                          for _ in range(max(2, int(pairs)))]

    def pending_packed(self) -> List[torch.Tensor]:
        """Host views (header + payloads) of the staged, uncommitted
        batches, oldest first."""
        return [b.pair.host[:b.used] for b in self._pk_pending]

    def _pk_open(self) -> Optional[_PackedBatch]:
        for p in self._pk_pairs:
            if not p.free and p.scattered and p.done_event.query():
                p.free, p.scattered = True, False
        for p in self._pk_pairs:
            if p.free:
                p.free = False
                return _PackedBatch(p, self._pk_hdr_words, self.num_tasks,
                                    list(self._pk_wp), list(self._pk_size))
        return None

    def _pk_abort(self, b: _PackedBatch) -> None:
        self._pk_wp, self._pk_size = b.wp0, b.size0
        b.pair.free = True

    def _pk_add(self, b: _PackedBatch, task: int, n: int, off: int) -> None:
        """Descriptor for one staged block: assigns its write pointer."""
        cap = self.shards[0].capacity
        if not 0 <= task < self.num_tasks:
            raise ValueError(f"packed block: task {task} out of range "
                             f"[0, {self.num_tasks})")
        rows = min(n, cap)        # keep only the newest `capacity` rows
        dst = self._pk_wp[task]
        b.desc += (task, n, n - rows, rows, off, dst, b.rows, 0)
        b.n_desc += 1
        b.rows += rows
        b.rows_t[task] += rows
        self._pk_wp[task] = (dst + rows) % cap
        self._pk_size[task] = min(self._pk_size[task] + rows, cap)

    def _pk_close(self, b: _PackedBatch) -> None:
        """Write the header and start the H2D copy on the copy stream."""
        from ..ops import torch_ref
        if b.n_desc == 0:
            b.pair.free = True
            return
        T, pair = self.num_tasks, b.pair
        b.used = b.off
        b.post_wp, b.post_size = list(self._pk_wp), list(self._pk_size)
        h0 = torch_ref.PK_HDR
        pair.host_i32[:h0] = torch.tensor([b.n_desc, T, b.rows, b.used],
                                          dtype=torch.int32)
        pair.host[h0:h0 + T] = torch.tensor(b.post_size, dtype=torch.float32)
        pair.host_i32[h0 + T:h0 + T + len(b.desc)] = torch.tensor(
            b.desc, dtype=torch.int32)
        if self.device.type == "cuda":
            with torch.cuda.stream(self._pk_copy_stream):
                pair.dev[:b.used].copy_(pair.host[:b.used], non_blocking=True)
                pair.copy_event.record(self._pk_copy_stream)
        self._pk_pending.append(b)

    @torch.no_grad()
    def stage_packed(self, rings=None, blocks=None,
                     max_blocks: int = 64) -> int:
        """Pack pending blocks into staging pairs and start their H2D
        copies.  Give either ``rings`` (native ShmRing objects; up to
        ``max_blocks`` per ring are drained with ``pop_into``) or ``blocks``
        (an iterable of ``(task, states, actions, rewards, next_states,
        dones)`` host tensors).  A new batch starts whenever a pair fills
        or one task's rows in the batch would exceed the shard capacity
        (no two rows of one launch share a destination).  Stops when no
        pair is free — unstaged blocks stay in their ring / with the
        caller.  Returns the number of blocks taken."""
        if (rings is None) == (blocks is None):
            raise ValueError("give exactly one of rings= / blocks=")
        if blocks is not None:
            blocks = list(blocks)
            for blk in blocks:   # reject bad input before any packing
                if not 0 <= int(blk[0]) < self.num_tasks:
                    raise ValueError(f"packed block: task {int(blk[0])} out "
                                     f"of range [0, {self.num_tasks})")
        if not self._pk_pairs:
            if rings is not None:
                slot = max((int(r.slot_floats()) for r in rings), default=0)
                self.configure_packed(max(slot, min(256 * slot, 1 << 23)))
            else:
                need = max((b[1].shape[0] for b in blocks), default=0)
                self.configure_packed(max(1 << 16,
                                          4 * need * self._row_floats))
        if not self._pk_pending:   # shards may have moved via append()
            self._pk_wp = [s.write_ptr for s in self.shards]
            self._pk_size = [s.size for s in self.shards]
        b: Optional[_PackedBatch] = None
        taken = 0
        try:
            if blocks is not None:
                taken, b = self._pk_stage_blocks(blocks)
            else:
                taken, b = self._pk_stage_rings(rings, max_blocks)
        except BaseException:
            # roll the staged-view pointers back to the last closed batch
            if self._pk_open_batch is not None:
                self._pk_abort(self._pk_open_batch)
                self._pk_open_batch = None
            raise
        if b is not None:
            self._pk_close(b)
        self._pk_open_batch = None
        return taken

    def _pk_stage_blocks(self, blocks):
        cap, rf = self.shards[0].capacity, self._row_floats
        limit = self._pk_pairs[0].host.numel()
        Ds, Da = self.f_states.shape[2], self.f_actions.shape[2]
        b, taken = None, 0
        for task, s, a, r, ns, d in blocks:
            task, n = int(task), s.shape[0]
            if n == 0:
                taken += 1
                continue
            need = n * rf
            if self._pk_hdr_words + need > limit:
                raise ValueError("packed block larger than a staging buffer")
            if b is not None and (b.off + need > limit
                                  or b.n_desc >= self._pk_max_desc
                                  or b.rows_t[task] + min(n, cap) > cap):
                self._pk_close(b)
                b = self._pk_open_batch = None
            if b is None:
                b = self._pk_open_batch = self._pk_open()
                if b is None:
                    break
            o = b.off
            for src, w in ((s, Ds), (a, Da), (r, 1), (ns, Ds), (d, 1)):
                b.pair.host[o:o + n * w].copy_(src.reshape(-1))
                o += n * w
            self._pk_add(b, task, n, b.off)
            b.off = o
            taken += 1
        return taken, b

    def _pk_stage_rings(self, rings, max_blocks):
        cap, rf = self.shards[0].capacity, self._row_floats
        b, taken = None, 0
        for ring in rings:
            left = max_blocks
            while left > 0:
                pend = int(ring.pending())
                if pend == 0:
                    break
                if b is None:
                    b = self._pk_open_batch = self._pk_open()
                    if b is None:
                        return taken, None
                k = min(left, pend, self._pk_max_desc - b.n_desc)
                got = ring.pop_into(b.pair.host, b.off, k,
                                    [cap - x for x in b.rows_t], cap) \
                    if k > 0 else []
                for task, n, off in got:
                    b.off = off + n * rf
                    if n:
                        self._pk_add(b, task, n, off)
                taken += len(got)
                left -= len(got)
                if len(got) < k or k <= 0:
                    # the next block did not fit this batch (space,
                    # descriptor count or its task's row budget)
                    if not got and b.off == self._pk_hdr_words:
                        raise RuntimeError(
                            "ring block larger than a staging buffer")
                    self._pk_close(b)
                    b = self._pk_open_batch = None
        return taken, b

    def _pk_scatter(self, b: _PackedBatch) -> None:
        from ..ops import native, native_enabled, torch_ref
        pair = b.pair
        fields = (self.f_states, self.f_actions, self.f_rewards,
                  self.f_next_states, self.f_dones, self.sizes_dev)
        if self.device.type == "cuda" and native_enabled():
            # host re-validation + launch on the current (main) stream
            native().replay_ingest(pair.dev, pair.host[:self._pk_hdr_words],
                                   *fields)
            if self.per_prio is not None:
                native().per_ingest_packed(
                    pair.dev, pair.host[:self._pk_hdr_words],
                    *self._per_state(), self._per_ws)
            pair.done_event.record()
            pair.scattered = True
        else:
            torch_ref.replay_ingest(pair.host[:b.used], *fields)
            if self.per_prio is not None:
                T, cap, Ds = self.f_states.shape
                for d in torch_ref.packed_validate(
                        pair.host[:b.used], T, cap, Ds,
                        self.f_actions.shape[2]):
                    torch_ref.per_ingest_(*self._per_state(), d[0], d[5],
                                          d[3])
            pair.free = True
        for t, shard in enumerate(self.shards):
            shard.write_ptr, shard.size = b.post_wp[t], b.post_size[t]

    @torch.no_grad()
    def commit_packed(self) -> int:
        """Launch the scatter for every staged batch whose H2D copy has
        completed (in order; a batch still copying blocks the ones behind
        it until the next call).  Returns the rows committed."""
        rows = 0
        while self._pk_pending:
            b = self._pk_pending[0]
            if b.pair.copy_event is not None \
                    and not b.pair.copy_event.query():
                break
            try:
                self._pk_scatter(b)
            except BaseException:
                # a rejected batch poisons everything staged behind it
                for x in self._pk_pending:
                    x.pair.free = True
                self._pk_pending.clear()
                raise
            self._pk_pending.pop(0)
            rows += b.rows
            self.packed_batches += 1
        return rows

    @torch.no_grad()
    def flush_packed(self) -> int:
        """Wait for every pending batch's copy and commit it."""
        rows = 0
        while self._pk_pending:
            ev = self._pk_pending[0].pair.copy_event
            if ev is not None:
                ev.synchronize()
            rows += self.commit_packed()
        return rows

    @torch.no_grad()
    def append_numpy(self, states, actions, rewards, next_states, dones,
                     task_idx: int = 0) -> None:
        """Ingest a block of host transitions into one task shard."""
        self.flush_packed()
        s = self._stage("s", states)
        a = self._stage("a", actions)
        r = self._stage("r", np.asarray(rewards).reshape(-1, 1))
        ns = self._stage("ns", next_states)
        d = self._stage("d", np.asarray(dones, dtype=np.float32).reshape(-1, 1))
        self.shards[task_idx].append(s, a, r, ns, d)

    @torch.no_grad()
    def append(self, task_idx: int, **fields: torch.Tensor) -> None:
        self.flush_packed()
        self.shards[task_idx].append(
            fields["states"], fields["actions"], fields["rewards"],
            fields["next_states"], fields["dones"])

    @torch.no_grad()
    def sample_indices_norepl(self, batch_size: int) -> torch.Tensor:
        """In-shard indices of one without-replacement draw (the torch
        oracle): int64 ``[T * (batch_size // T)]``, shard-major.  Keyed by
        the attached rng counter if there is one, otherwise by an int64
        drawn from this replay's generator per call."""
        from ..ops import torch_ref
        ctr = self._rng_ctr
        if ctr is None:
            ctr = torch.randint(0, 1 << 62, (1,), device=self.device,
                                generator=self.generator)
        return torch_ref.replay_sample_indices_norepl(
            self.sizes_dev, batch_size, self.num_tasks, ctr)

    def _sample_norepl(self, batch_size: int,
                       graph_safe: bool) -> Dict[str, torch.Tensor]:
        T = self.num_tasks
        fields = (self.f_states, self.f_actions, self.f_rewards,
                  self.f_next_states, self.f_dones)
        if graph_safe and self.device.type == "cuda" \
                and batch_size % T == 0:
            from ..ops import native, native_enabled
            if native_enabled():
                if self._rng_ctr is None:
                    raise RuntimeError(
                        "sampling='without_replacement' draws its graph-safe "
                        "batches in k_replay_sample_norepl, which needs the "
                        "engine's device rng counter: call attach_rng() "
                        "(engine.capture does) and leave DSAC_KRNG at 1")
                o = native().replay_sample_norepl(
                    *fields, self.sizes_dev, batch_size, self._rng_ctr)
                return dict(zip(FIELDS, o))
        per = batch_size // T
        cap = self.f_states.shape[1]
        idx = self.sample_indices_norepl(batch_size)
        idx += torch.arange(T, device=self.device).repeat_interleave(per) * cap
        if not graph_safe and T > 1:   # the reference's shuffled concat
            idx = idx[torch.randperm(per * T, device=self.device,
                                     generator=self.generator)]
        return {name: f.reshape(T * cap, -1).index_select(0, idx)
                for name, f in zip(FIELDS, fields)}

    def _sample_per(self, batch_size: int,
                    graph_safe: bool) -> Dict[str, torch.Tensor]:
        """Prioritized draw: the five fields plus ``indices`` (flat row
        indices, int64 ``[B]``) and ``is_weights`` (raw, fp32 ``[B]``).
        Rows are shard-major on every path (no concat shuffle)."""
        T = self.num_tasks
        cap = self.f_states.shape[1]
        fields = (self.f_states, self.f_actions, self.f_rewards,
                  self.f_next_states, self.f_dones)
        if graph_safe and self.device.type == "cuda" \
                and batch_size % T == 0:
            from ..ops import native, native_enabled
            if native_enabled():
                if self._rng_ctr is None:
                    raise RuntimeError(
                        "sampling='prioritized' draws its graph-safe "
                        "batches in k_replay_sample_per, which needs the "
                        "engine's device rng counter: call attach_rng() "
                        "(engine.capture does) and leave DSAC_KRNG at 1")
                if batch_size > 8192:
                    raise NotImplementedError(
                        "sampling='prioritized': batches above 8192 rows "
                        "are not supported on the GPU path")
                idx = torch.empty(batch_size, dtype=torch.int64,
                                  device=self.device)
                w = torch.empty(batch_size, device=self.device)
                o = native().replay_sample_per(
                    *fields, self.sizes_dev, self.per_prio, self.per_bsum,
                    self.per_total, self.per_beta, batch_size,
                    self._rng_ctr, idx, w)
                out = dict(zip(FIELDS, o))
                out["indices"], out["is_weights"] = idx, w
                return out
        from ..ops import torch_ref
        per = batch_size // T
        ctr = self._rng_ctr
        if ctr is None:
            ctr = torch.randint(0, 1 << 62, (1,), device=self.device,
                                generator=self.generator)
        idx = torch_ref.per_sample_indices(
            self.per_prio, self.per_bsum, self.per_total, self.sizes_dev,
            batch_size, T, ctr)
        w = torch_ref.per_is_weights(self.per_prio, self.per_total,
                                     self.sizes_dev, idx, self.per_beta)
        idx = idx + torch.arange(T, device=self.device) \
            .repeat_interleave(per) * cap
        out = {name: f.reshape(T * cap, -1).index_select(0, idx)
               for name, f in zip(FIELDS, fields)}
        out["indices"], out["is_weights"] = idx, w
        return out

    @torch.no_grad()
    def sample(self, batch_size: int,
               graph_safe: bool = False) -> Dict[str, torch.Tensor]:
        """Stratified across shards, shuffled concat (reference
        replay_buffers.sample:67-100); single shard = plain uniform.

        graph_safe=True uses the hipGraph-capturable index draw and skips
        the concat shuffle (every consumer of the batch is
        permutation-invariant: all losses are batch means).

        Pending packed batches are flushed first, so the host-side sizes
        the non-graph draw uses match what is in device memory.

        With ``sampling="without_replacement"`` each shard's rows are
        distinct (while the shard holds at least ``batch_size //
        num_tasks`` rows): graph_safe=True on a GPU draws in
        ``k_replay_sample_norepl``, every other path with the same
        algorithm in torch.

        With ``sampling="prioritized"`` rows are drawn in proportion to
        their priorities (``k_replay_sample_per`` for graph_safe=True on a
        GPU, ``torch_ref.per_sample_indices`` elsewhere) and the batch
        carries two more keys, ``indices`` and ``is_weights``; feed the
        update's new priorities to :meth:`update_priorities`."""
        if self._pk_pending:
            self.flush_packed()
        if self.sampling == "without_replacement":
            return self._sample_norepl(batch_size, graph_safe)
        if self.sampling == "prioritized":
            return self._sample_per(batch_size, graph_safe)
        gen = None if graph_safe else self.generator
        if graph_safe and self.device.type == "cuda":
            from ..ops import has_native, native, native_enabled
            if native_enabled() and has_native() \
                    and batch_size % self.num_tasks == 0:
                if self._rng_ctr is not None:
                    # counter-based in-kernel uniforms: no torch.rand
                    # launch, no graph RNG-offset bookkeeping kernels
                    if self._empty_rnd is None:
                        self._empty_rnd = torch.empty(
                            0, device=self.device)
                    o = native().replay_sample(
                        self.f_states, self.f_actions, self.f_rewards,
                        self.f_next_states, self.f_dones, self.sizes_dev,
                        self._empty_rnd, batch_size, self._rng_ctr)
                    return dict(zip(FIELDS, o))
                rnd = torch.rand(batch_size, device=self.device)
                o = native().replay_sample(
                    self.f_states, self.f_actions, self.f_rewards,
                    self.f_next_states, self.f_dones, self.sizes_dev, rnd,
                    batch_size)
                return dict(zip(FIELDS, o))
        if self.num_tasks == 1:
            return self.shards[0].sample(batch_size, gen, graph_safe)
        per = batch_size // self.num_tasks
        parts = [s.sample(per, gen, graph_safe) for s in self.shards]
        out: Dict[str, torch.Tensor] = {}
        perm = None
        if not graph_safe:
            perm = torch.randperm(per * self.num_tasks, device=self.device,
                                  generator=gen)
        for f in FIELDS:
            cat = torch.cat([p[f] for p in parts], dim=0)
            out[f] = cat.index_select(0, perm) if perm is not None else cat
        return out
