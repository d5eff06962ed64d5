"""Packed replay ingest: ring -> one staging buffer -> one H2D copy -> one
k_replay_ingest scatter, checked bit-exactly against the per-block path
(``ReplayShard.append``).  The path only moves floats, so every equality
is ``torch.equal``.

Rule under test for mixed use: ``append`` / ``append_numpy`` / ``sample``
on a replay with uncommitted packed batches FLUSH them first.
"""

import os
import queue

import pytest
import torch

from distributed_sac_amd.ops import torch_ref
from distributed_sac_amd.replay import ShardedReplay

T, CAP, DA = 3, 8, 2
DS_CASES = (5, 70)     # < 64 lanes and not a multiple of 4; > 64 columns
FIELD_ATTRS = ("f_states", "f_actions", "f_rewards", "f_next_states",
               "f_dones")

# (task, rows).  Covers: two blocks of one task in a batch (0,3)(0,3); a
# wrap inside one block (third (0,3) lands at write_ptr 6); a run whose
# per-task total exceeds cap (task 0: 3+3+3, task 1: 1+8+11) so the host
# must split; rows == cap (8) and rows > cap (11, trimmed to the newest 8);
# task 2 receives nothing.
SEQ = ((0, 3), (1, 1), (0, 3), (0, 3), (1, 8), (1, 11), (0, 1), (1, 3),
       (0, 8), (0, 3))
ROWS_PUSHED = sum(n for _, n in SEQ)
ROWS_TRIMMED = sum(max(0, n - CAP) for _, n in SEQ)


def make_blocks(ds, seq=SEQ, seed=0):
    """Seeded host blocks; every row carries a unique positive reward."""
    g = torch.Generator().manual_seed(seed)
    blocks, marker = [], 1
    for task, n in seq:
        r = torch.arange(marker, marker + n, dtype=torch.float32)
        marker += n
        blocks.append((task, torch.randn(n, ds, generator=g),
                       torch.randn(n, DA, generator=g), r.reshape(n, 1),
                       torch.randn(n, ds, generator=g),
                       (torch.rand(n, 1, generator=g) < 0.3).float()))
    return blocks


def new_replay(ds, device="cpu"):
    r = ShardedReplay(T * CAP, T, ds, DA, device=device)
    r.f_rewards.fill_(-1.0)      # untouched storage carries a negative mark
    return r


def feed_blocks(replay, blocks):
    """The per-block reference path."""
    for task, s, a, r, ns, d in blocks:
        replay.shards[task].append(s, a, r, ns, d)


def feed_packed(replay, blocks):
    """stage until everything is taken, flushing when no pair is free."""
    i = 0
    while i < len(blocks):
        took = replay.stage_packed(blocks=blocks[i:])
        i += took
        if took == 0:
            assert replay.flush_packed() > 0
    replay.flush_packed()


def assert_same(a, b):
    if a.device.type == "cuda":
        torch.cuda.synchronize()
    for f in FIELD_ATTRS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert torch.equal(a.sizes_dev, b.sizes_dev)
    for sa, sb in zip(a.shards, b.shards):
        assert (sa.size, sa.write_ptr, len(sa)) == \
            (sb.size, sb.write_ptr, len(sb))
    assert len(a) == len(b) and a.total_size == b.total_size


def make_ring(tag, ds, n_slots=16):
    from distributed_sac_amd import ops
    ext = ops.native()
    return ext.ShmRing(f"/dsac_pk_{tag}_{os.getpid()}", n_slots,
                       11 * (2 * ds + DA + 2), ds, DA)


def decode_payload(staging, n, off, ds):
    out, o = [], off
    for w in (ds, DA, 1, ds, 1):
        out.append(staging[o:o + n * w].reshape(n, w))
        o += n * w
    return out


# -- CPU ------------------------------------------------------------------

@pytest.mark.parametrize("ds", DS_CASES)
def test_packed_cpu_matches_per_block(ds):
    blocks = make_blocks(ds)
    ref, pk = new_replay(ds), new_replay(ds)
    feed_blocks(ref, blocks)
    pk.configure_packed(1 << 12, pairs=8)     # a pair per batch needed
    taken = pk.stage_packed(blocks=blocks)
    assert taken == len(blocks)
    # the per-task totals exceed cap, so the host split the sequence
    assert len(pk.pending_packed()) == 5
    assert pk.packed_batches == 0
    # host-visible state moves at commit, not at stage
    assert pk.total_size == 0 and len(pk) == 0
    assert all(s.write_ptr == 0 for s in pk.shards)
    assert torch.equal(pk.sizes_dev, torch.zeros(T))
    assert pk.flush_packed() == ROWS_PUSHED - ROWS_TRIMMED
    assert pk.packed_batches == 5
    assert pk.shards[2].size == 0          # the task that received nothing
    assert_same(pk, ref)


def test_packed_batches_never_alias_a_row():
    pk = new_replay(5)
    pk.stage_packed(blocks=make_blocks(5))
    for buf in pk.pending_packed():
        descs = torch_ref.packed_validate(buf, T, CAP, 5, DA)
        per_task = [0] * T
        for task, _n, _first, rows, *_ in descs:
            per_task[task] += rows
        assert max(per_task) <= CAP


def test_out_of_range_task_raises_before_any_write():
    pk = new_replay(5)
    blocks = make_blocks(5)[:2]
    bad = (T,) + blocks[1][1:]
    before = [getattr(pk, f).clone() for f in FIELD_ATTRS]
    with pytest.raises(ValueError):
        pk.stage_packed(blocks=[blocks[0], bad])
    assert pk.pending_packed() == [] and pk.flush_packed() == 0
    # the same through a forged header on an otherwise good batch
    pk.stage_packed(blocks=blocks)
    buf = pk.pending_packed()[0]
    buf.view(torch.int32)[torch_ref.PK_HDR + T] = T
    with pytest.raises(ValueError):
        pk.commit_packed()
    for f, b in zip(FIELD_ATTRS, before):
        assert torch.equal(getattr(pk, f), b)
    assert pk.total_size == 0 and torch.equal(pk.sizes_dev, torch.zeros(T))
    # the replay stays usable
    good, ref = make_blocks(5), new_replay(5)
    feed_blocks(ref, good)
    feed_packed(pk, good)
    assert_same(pk, ref)


@pytest.mark.parametrize("word,value", [(4, 1 << 20),    # payload offset
                                        (1, 1 << 12),    # block row count
                                        (3, CAP + 1)])   # rows > cap
def test_extent_past_staging_raises_before_any_write(word, value):
    pk = new_replay(5)
    pk.stage_packed(blocks=make_blocks(5)[:2])
    buf = pk.pending_packed()[0]
    buf.view(torch.int32)[torch_ref.PK_HDR + T + word] = value
    before = [getattr(pk, f).clone() for f in FIELD_ATTRS]
    with pytest.raises(ValueError):
        pk.commit_packed()
    for f, b in zip(FIELD_ATTRS, before):
        assert torch.equal(getattr(pk, f), b)
    assert pk.total_size == 0


def test_header_used_past_buffer_raises():
    pk = new_replay(5)
    pk.stage_packed(blocks=make_blocks(5)[:2])
    buf = pk.pending_packed()[0].clone()
    buf.view(torch.int32)[3] = buf.numel() + 1
    with pytest.raises(ValueError):
        torch_ref.replay_ingest(buf, pk.f_states, pk.f_actions, pk.f_rewards,
                                pk.f_next_states, pk.f_dones, pk.sizes_dev)
    assert float(pk.f_rewards.max()) == -1.0


def test_append_and_sample_flush_uncommitted_batches():
    blocks = make_blocks(5)
    extra = make_blocks(5, seq=((2, 3),), seed=1)[0]
    ref = new_replay(5)
    feed_blocks(ref, blocks[:3] + [extra])

    pk = new_replay(5)
    pk.stage_packed(blocks=blocks[:3])
    assert pk.total_size == 0
    pk.append(2, states=extra[1], actions=extra[2], rewards=extra[3],
              next_states=extra[4], dones=extra[5])
    assert pk.pending_packed() == []
    assert_same(pk, ref)

    pk = new_replay(5)
    pk.stage_packed(blocks=blocks[:3])
    pk.append_numpy(extra[1].numpy(), extra[2].numpy(), extra[3].numpy(),
                    extra[4].numpy(), extra[5].numpy(), task_idx=2)
    assert_same(pk, ref)

    pk = new_replay(5)
    pk.stage_packed(blocks=blocks[:3] + [extra])
    out = pk.sample(6)
    assert pk.pending_packed() == [] and pk.total_size == ref.total_size
    assert float(out["rewards"].min()) > 0    # only ingested rows


def test_ring_pop_into():
    from distributed_sac_amd import ops
    if not ops.has_native():
        pytest.skip("native extension not built")
    ds = 5
    rf = 2 * ds + DA + 2
    blocks = make_blocks(ds)
    ring = make_ring("pop", ds)
    for b in blocks:
        assert ring.push(*b)
    # room for everything: payloads come back as pushed, back to back
    big = torch.full((7 + ROWS_PUSHED * rf,), -7.0)
    got = ring.pop_into(big, 7, 64)
    assert ring.pending() == 0 and len(got) == len(blocks)
    off = 7
    for (task, n, o), b in zip(got, blocks):
        assert (task, n, o) == (b[0], b[1].shape[0], off)
        for x, y in zip(decode_payload(big, n, o, ds), b[1:]):
            assert torch.equal(x, y)
        off += n * rf
    assert torch.equal(big[:7], torch.full((7,), -7.0))

    # too small for all: returns early, the rest stays pending, in order
    for b in blocks:
        assert ring.push(*b)
    fit = sum(n for _, n in SEQ[:4]) * rf
    small = torch.zeros(fit + SEQ[4][1] * rf - 1)   # block 4 misses by one
    first = ring.pop_into(small, 0, 64)
    assert [(t, n) for t, n, _ in first] == list(SEQ[:4])
    assert ring.pending() == len(SEQ) - 4
    rest = ring.pop_into(big, 0, 64)
    assert [(t, n) for t, n, _ in rest] == list(SEQ[4:])
    assert ring.pending() == 0
    for (task, n, o), b in zip(rest, blocks[4:]):
        for x, y in zip(decode_payload(big, n, o, ds), b[1:]):
            assert torch.equal(x, y)
    # max_blocks and the per-task row budget both stop without consuming
    for b in blocks[:4]:
        assert ring.push(*b)
    assert len(ring.pop_into(big, 0, 1)) == 1
    got = ring.pop_into(big, 0, 64, [3, CAP, CAP], CAP)
    assert [(t, n) for t, n, _ in got] == [(1, 1), (0, 3)]
    assert ring.pending() == 1
    assert len(ring.pop_into(big, 0, 64)) == 1


def test_ring_stage_packed_cpu():
    """rings -> stage_packed -> torch_ref decode, against the block path."""
    from distributed_sac_amd import ops
    if not ops.has_native():
        pytest.skip("native extension not built")
    ds = 5
    blocks = make_blocks(ds)
    rings = [make_ring("st0", ds), make_ring("st1", ds)]
    ref, pk = new_replay(ds), new_replay(ds)
    # drain order is ring 0 then ring 1
    for b in blocks[:6]:
        assert rings[0].push(*b)
    for b in blocks[6:]:
        assert rings[1].push(*b)
    feed_blocks(ref, blocks)
    taken = 0
    while any(r.pending() for r in rings):
        got = pk.stage_packed(rings=rings)
        taken += got
        if got == 0:
            pk.flush_packed()
    assert taken == len(blocks)
    pk.flush_packed()
    assert_same(pk, ref)


def test_learner_rejects_unknown_ingest_mode():
    from distributed_sac_amd.workers.learner import Learner
    from distributed_sac_amd.workers.param_server import ParamSnapshot
    from tests.test_engine import small_cfg
    with pytest.raises(ValueError):
        Learner(small_cfg("mtsac"), "cpu", ParamSnapshot(8), queue.Queue(),
                ingest="bogus")


# -- GPU ------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ds", DS_CASES)
def test_replay_ingest_kernel_matches_per_block(ds):
    blocks = make_blocks(ds)
    ref, pk = new_replay(ds, "cuda:0"), new_replay(ds, "cuda:0")
    feed_blocks(ref, blocks)
    feed_packed(pk, blocks)
    assert_same(pk, ref)


@pytest.mark.gpu
def test_staging_pairs_are_reused():
    """More batches than staging pairs: every pair carries several
    batches, each reused only after its scatter has completed."""
    ds = 70
    blocks = make_blocks(ds) + make_blocks(ds, seed=3)
    ref, pk = new_replay(ds, "cuda:0"), new_replay(ds, "cuda:0")
    # room for ONE 11-row block per batch, two pairs
    pk.configure_packed(11 * (2 * ds + DA + 2), max_desc=4, pairs=2)
    feed_blocks(ref, blocks)
    feed_packed(pk, blocks)
    assert pk.packed_batches > 2 * 2      # every pair carried > 2 batches
    assert_same(pk, ref)


@pytest.mark.gpu
def test_bad_descriptor_never_reaches_the_kernel():
    pk = new_replay(5, "cuda:0")
    pk.stage_packed(blocks=make_blocks(5)[:2])
    buf = pk.pending_packed()[0]
    buf.view(torch.int32)[torch_ref.PK_HDR + T] = T      # task out of range
    with pytest.raises(RuntimeError):
        pk.flush_packed()
    torch.cuda.synchronize()
    assert float(pk.f_rewards.max()) == -1.0
    assert pk.total_size == 0


@pytest.mark.gpu
def test_native_sampler_sees_only_ingested_rows():
    from distributed_sac_amd import ops
    ops.native()
    ds = 5
    blocks = make_blocks(ds, seq=SEQ[:4] + ((2, 1),))    # every task fed
    pk = new_replay(ds, "cuda:0")
    feed_packed(pk, blocks)
    out = pk.sample(96, graph_safe=True)
    torch.cuda.synchronize()
    assert out["rewards"].shape == (96, 1)
    assert float(out["rewards"].min()) > 0
    ingested = torch.cat([b[3] for b in blocks]).flatten().tolist()
    assert set(out["rewards"].flatten().tolist()) <= set(ingested)


@pytest.mark.gpu
def test_learner_packed_matches_blocks():
    from distributed_sac_amd.workers.learner import Learner
    from distributed_sac_amd.workers.param_server import ParamSnapshot
    from tests.test_engine import small_cfg
    cfg = small_cfg("mtsac")
    cfg.num_tasks, cfg.state_dim, cfg.action_dim = T, 2, DA
    cfg.buffer_size = T * CAP
    ds = cfg.mtobs_dim
    blocks = make_blocks(ds)
    learners = {}
    for mode in ("blocks", "packed"):
        ring = make_ring(f"lr_{mode}", ds)
        for b in blocks:
            assert ring.push(*b)
        lr = Learner(cfg, "cuda:0", ParamSnapshot(8), queue.Queue(),
                     rings=[ring], precision="fp32", use_graph=False,
                     ingest=mode)
        assert lr.ingest == mode
        while ring.pending():
            lr.drain_rings()
        lr.flush_packed()
        learners[mode] = lr
    torch.cuda.synchronize()
    pk, ref = learners["packed"], learners["blocks"]
    assert pk.ingest_count == ROWS_PUSHED - ROWS_TRIMMED
    assert pk.engine.total_step == pk.ingest_count
    assert_same(pk.replay, ref.replay)
