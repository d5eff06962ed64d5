"""Opt-in without-replacement replay sampling
(``sampling="without_replacement"``): the keyed-permutation draw of
``torch_ref.replay_sample_indices_norepl`` (CPU path and exact oracle), its
HIP twin ``k_replay_sample_norepl``, and the plumbing from ``SACConfig`` /
``Learner`` down to ``ShardedReplay``.

The chi-square bounds are p > 1e-4 per test (Bonferroni over the 16 row
positions / the five sizes); the draws are deterministic functions of the
counters used here, so the tests cannot flake."""

import glob
import os
import queue

import pytest
import torch

from distributed_sac_amd.config import SACConfig
from distributed_sac_amd.ops import torch_ref
from distributed_sac_amd.replay import ShardedReplay

T3, CAP, DA = 3, 64, 2
SIZES = (40, 64, 17)
NOREPL = "without_replacement"


def fill(r: ShardedReplay, sizes, seed: int = 0) -> None:
    """``sizes[t]`` rows into shard t; reward = 1000 t + row, unique."""
    g = torch.Generator().manual_seed(seed)
    ds, da = r.f_states.shape[2], r.f_actions.shape[2]
    for t, n in enumerate(sizes):
        if n == 0:
            continue
        r.append(t, states=torch.randn(n, ds, generator=g).to(r.device),
                 actions=torch.randn(n, da, generator=g).to(r.device),
                 rewards=(1000.0 * t + torch.arange(n)).reshape(n, 1)
                 .to(r.device),
                 next_states=torch.randn(n, ds, generator=g).to(r.device),
                 dones=(torch.rand(n, 1, generator=g) < 0.3).float()
                 .to(r.device))


def make_replay(sizes=SIZES, ds=5, device="cpu", cap=CAP, **kw):
    T = len(sizes)
    r = ShardedReplay(T * cap, T, ds, DA, device=device, **kw)
    fill(r, sizes)
    return r


def chi2_pvalue(counts: torch.Tensor) -> float:
    """Upper tail of the chi-square test of ``counts`` against uniform."""
    c = counts.double()
    e = c.sum() / c.numel()
    stat = ((c - e) ** 2 / e).sum()
    df = torch.tensor(c.numel() - 1.0, dtype=torch.float64)
    return float(torch.special.gammaincc(df / 2, stat / 2))


def many_counters(n: int, per: int, K: int = 20000, base: int = 1000):
    """[K, per] indices of shard 0 for K consecutive counters."""
    return torch_ref.norepl_index(
        torch.tensor(n), torch.tensor(0), torch.arange(per)[None, :],
        torch.arange(K)[:, None] + base)


# -- CPU ------------------------------------------------------------------

def test_bijective_for_every_size():
    longest = 0
    for n in list(range(1, 301)) + [1023, 1024, 1025, 4097, 100000]:
        for ctr in (0, 7, 123456789):
            idx = torch_ref.replay_sample_indices_norepl([n], n, 1, ctr)
            assert idx.dtype == torch.int64 and idx.shape == (n,)
            assert torch.equal(idx.sort().values, torch.arange(n)), (n, ctr)
    # the walk lengths docs/KERNELS.md records
    for n in (2, 33, 65, 100000):
        N = torch.full((n,), n)
        _, walk = torch_ref.norepl_index(
            N, torch.zeros_like(N), torch.arange(n), torch.zeros_like(N),
            return_walk=True)
        assert int(walk.min()) >= 1
        assert int(walk.max()) <= (1 << max(6, (n - 1).bit_length())) - n + 1
        longest = max(longest, int(walk.max()))
    print("longest walk", longest)


@pytest.mark.parametrize("graph_safe", [False, True])
def test_rows_distinct_and_from_their_shard(graph_safe):
    r = make_replay(sampling=NOREPL, seed=3)
    assert r.sampling == NOREPL
    for _ in range(5):
        rew = r.sample(48, graph_safe=graph_safe)["rewards"].reshape(-1)
        for t, n in enumerate(SIZES):
            mine = rew[(rew >= 1000 * t) & (rew < 1000 * (t + 1))]
            assert mine.numel() == 16                 # stratified
            assert mine.unique().numel() == 16        # distinct
            assert float(mine.max()) < 1000 * t + n   # rows that exist
        if graph_safe:   # shard-major, no shuffle
            assert torch.equal((rew // 1000).long(),
                               torch.arange(3).repeat_interleave(16))


def test_default_mode_does_repeat_rows():
    """Same shapes, default mode: some seed among 20 repeats a row, so the
    distinctness test above can tell the modes apart."""
    dup = 0
    for seed in range(20):
        r = make_replay(seed=seed)
        assert r.sampling == "replace"
        rew = r.sample(48)["rewards"].reshape(-1)
        dup += int(rew.unique().numel() < 48)
    assert dup >= 1


def test_whole_batch_matches_oracle_gather():
    """CPU sample() with an attached counter = index_select at the
    oracle's indices, field by field."""
    r = make_replay(sampling=NOREPL)
    ctr = torch.tensor([11], dtype=torch.int64)
    r.attach_rng(ctr)
    idx = torch_ref.replay_sample_indices_norepl(r.sizes_dev, 48, 3, ctr)
    assert torch.equal(idx, r.sample_indices_norepl(48))
    out = r.sample(48, graph_safe=True)
    for name, f in zip(("states", "actions", "rewards", "next_states",
                        "dones"),
                       (r.f_states, r.f_actions, r.f_rewards,
                        r.f_next_states, r.f_dones)):
        want = torch.cat([f[t].index_select(0, idx[16 * t:16 * t + 16])
                          for t in range(3)])
        assert torch.equal(out[name], want), name
    # a batch that does not divide: per = B // T rows per shard
    assert r.sample(50, graph_safe=True)["rewards"].shape == (48, 1)
    assert r.sample(50)["rewards"].shape == (48, 1)


def test_shard_smaller_than_its_share():
    sizes = (5, 64, 64)
    idx = torch_ref.replay_sample_indices_norepl(sizes, 48, 3, 5)
    for t, n in enumerate(sizes):
        part = idx[16 * t:16 * t + 16]
        assert int(part.min()) >= 0 and int(part.max()) < n
    cnt = torch.bincount(idx[:16], minlength=5)
    assert cnt.numel() == 5 and int(cnt.min()) >= 3 and int(cnt.max()) <= 4
    r = make_replay(sizes, sampling=NOREPL, seed=0)
    rew = r.sample(48, graph_safe=True)["rewards"].reshape(-1)[:16]
    cnt = torch.bincount(rew.long(), minlength=5)
    assert cnt.numel() == 5 and int(cnt.min()) >= 3 and int(cnt.max()) <= 4


def test_empty_shard_reads_row_zero():
    idx = torch_ref.replay_sample_indices_norepl((0, 64, 1), 48, 3, 9)
    assert int(idx[:16].abs().max()) == 0 and int(idx[32:].abs().max()) == 0
    assert idx[16:32].unique().numel() == 16


def test_marginals_uniform():
    idx = many_counters(100, 16)
    ps = [chi2_pvalue(torch.bincount(idx[:, p], minlength=100))
          for p in range(16)]
    print("marginal p-values", ["%.3g" % p for p in ps])
    assert min(ps) > 1e-4, ps


@pytest.mark.parametrize("n", [5, 8, 17, 64, 100])
def test_joint_uniform(n):
    idx = many_counters(n, 2)
    cnt = torch.bincount((idx[:, 1] - idx[:, 0]) % n, minlength=n)
    assert int(cnt[0]) == 0           # the two rows never coincide
    p = chi2_pvalue(cnt[1:])
    print("joint p-value", n, p)
    assert p > 1e-4, (n, p)


def test_fresh_and_reproducible():
    draw = torch_ref.replay_sample_indices_norepl
    a = draw((64, 64, 64), 48, 3, 100)
    assert torch.equal(a, draw((64, 64, 64), 48, 3, 100))
    assert torch.equal(a, draw(torch.tensor([64., 64., 64.]), 48, 3,
                               torch.tensor([100])))
    assert not torch.equal(a, draw((64, 64, 64), 48, 3, 101))
    assert not torch.equal(a[:16], a[16:32])     # equal sizes, other shard
    assert not torch.equal(a[16:32], a[32:])
    # without a counter the key comes from the seeded generator
    r1, r2 = (make_replay((64, 64, 64), sampling=NOREPL, seed=5)
              for _ in range(2))
    i1 = r1.sample_indices_norepl(48)
    assert torch.equal(i1, r2.sample_indices_norepl(48))
    assert not torch.equal(i1, r1.sample_indices_norepl(48))


def test_mode_validation_and_env_default(monkeypatch):
    with pytest.raises(ValueError):
        ShardedReplay(192, 3, 5, DA, sampling="bogus")
    monkeypatch.setenv("DSAC_SAMPLING", NOREPL)
    assert ShardedReplay(192, 3, 5, DA).sampling == NOREPL
    assert ShardedReplay(192, 3, 5, DA, sampling="replace").sampling \
        == "replace"
    monkeypatch.setenv("DSAC_SAMPLING", "bogus")
    with pytest.raises(ValueError):
        ShardedReplay(192, 3, 5, DA)
    monkeypatch.delenv("DSAC_SAMPLING")
    assert ShardedReplay(192, 3, 5, DA).sampling == "replace"


def test_config_key_and_reference_cfgs():
    assert SACConfig().replay_sampling == "replace"
    c = SACConfig.from_dict({"replay_sampling": NOREPL})
    assert c.replay_sampling == NOREPL
    assert SACConfig.from_dict(c.raw).replay_sampling == NOREPL
    with pytest.raises(ValueError):
        SACConfig.from_dict({"replay_sampling": "bogus"})
    paths = sorted(glob.glob(os.path.join(
        os.path.dirname(__file__), "golden", "reference_cfg", "*.json")))
    assert len(paths) == 5
    for p in paths:
        cfg = SACConfig.from_file(p)
        assert "replay_sampling" not in cfg.raw
        assert cfg.replay_sampling == "replace"


def test_learner_passes_the_mode_down(monkeypatch):
    from distributed_sac_amd.workers.learner import Learner
    from distributed_sac_amd.workers.param_server import ParamSnapshot
    from tests.test_engine import small_cfg
    monkeypatch.delenv("DSAC_SAMPLING", raising=False)

    def learner(cfg, **kw):
        cfg.buffer_size = 400
        return Learner(cfg, "cpu", ParamSnapshot(8), queue.Queue(), **kw)

    cfg = small_cfg("mtsac")
    assert learner(cfg).replay.sampling == "replace"
    assert learner(cfg, sampling=NOREPL).replay.sampling == NOREPL
    with pytest.raises(ValueError):
        learner(cfg, sampling="bogus")
    cfg.replay_sampling = NOREPL
    assert learner(cfg).replay.sampling == NOREPL
    assert learner(cfg, sampling="replace").replay.sampling == "replace"
    monkeypatch.setenv("DSAC_SAMPLING", NOREPL)
    assert learner(small_cfg("mtsac")).replay.sampling == NOREPL


def test_trainer_trains_in_the_new_mode(monkeypatch):
    import math
    from distributed_sac_amd.workers import Trainer
    from tests.test_trainer import tiny_cfg
    monkeypatch.delenv("DSAC_SAMPLING", raising=False)
    torch.manual_seed(0)
    cfg = tiny_cfg("mtsac")
    assert Trainer(cfg, device="cpu", seed=1).replay.sampling == "replace"
    cfg.replay_sampling = NOREPL
    tr = Trainer(cfg, device="cpu", seed=1)
    assert tr.replay.sampling == NOREPL
    metrics = tr.train(env_steps_per_iter=40, updates_per_iter=1,
                       iterations=3)
    assert tr.engine.update_iteration >= 1
    assert math.isfinite(float(metrics["critic_loss"]))


# -- GPU ------------------------------------------------------------------

def _check_kernel(r: ShardedReplay, B: int, ctr_value: int) -> None:
    from distributed_sac_amd import ops
    T, cap = r.num_tasks, r.f_states.shape[1]
    per = B // T
    ctr = torch.tensor([ctr_value], dtype=torch.int64, device="cuda")
    idx_out = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    fields = (r.f_states, r.f_actions, r.f_rewards, r.f_next_states,
              r.f_dones)
    out = ops.native().replay_sample_norepl(*fields, r.sizes_dev, B, ctr,
                                            idx_out)
    want = torch_ref.replay_sample_indices_norepl(r.sizes_dev, B, T, ctr)
    assert torch.equal(idx_out, want), (B, ctr_value)
    assert torch.equal(
        idx_out.cpu(),
        torch_ref.replay_sample_indices_norepl(r.sizes_dev.cpu(), B, T,
                                               ctr_value))
    flat = want + torch.arange(T, device="cuda").repeat_interleave(per) * cap
    for o, f in zip(out, fields):
        assert torch.equal(o, f.reshape(T * cap, -1).index_select(0, flat))
    # idx_out is optional
    out2 = ops.native().replay_sample_norepl(*fields, r.sizes_dev, B, ctr)
    assert all(torch.equal(a, b) for a, b in zip(out, out2))


@pytest.mark.gpu
@pytest.mark.parametrize("ds", [5, 70])
@pytest.mark.parametrize("sizes", [SIZES, (1, 2, 63), (0, 64, 5)])
def test_kernel_equals_oracle(ds, sizes):
    r = make_replay(sizes, ds=ds, device="cuda")
    for B in (48, 3):
        for ctr_value in (0, 2_000_000_011):
            _check_kernel(r, B, ctr_value)


@pytest.mark.gpu
def test_kernel_equals_oracle_single_shard():
    r = make_replay((4095,), ds=5, device="cuda", cap=4096)
    _check_kernel(r, 1024, 77)
    idx = torch_ref.replay_sample_indices_norepl(r.sizes_dev, 1024, 1, 77)
    assert idx.unique().numel() == 1024


@pytest.mark.gpu
def test_kernel_host_validation():
    from distributed_sac_amd import ops
    r = make_replay(device="cuda")
    fields = (r.f_states, r.f_actions, r.f_rewards, r.f_next_states,
              r.f_dones)
    ctr = torch.tensor([1], dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError):    # batch must divide by T
        ops.native().replay_sample_norepl(*fields, r.sizes_dev, 47, ctr)
    with pytest.raises(RuntimeError):    # counter must be int64
        ops.native().replay_sample_norepl(*fields, r.sizes_dev, 48,
                                          ctr.float())
    with pytest.raises(RuntimeError):    # idx_out must hold B entries
        ops.native().replay_sample_norepl(
            *fields, r.sizes_dev, 48, ctr,
            torch.empty(47, dtype=torch.int64, device="cuda"))


@pytest.mark.gpu
def test_graph_safe_sample_needs_the_counter():
    r = make_replay(device="cuda", sampling=NOREPL)
    with pytest.raises(RuntimeError, match="attach_rng"):
        r.sample(48, graph_safe=True)
    ctr = torch.tensor([4], dtype=torch.int64, device="cuda")
    r.attach_rng(ctr)
    rew = r.sample(48, graph_safe=True)["rewards"].reshape(-1)
    assert rew.unique().numel() == 48
    # the torch path draws the same rows for the same counter
    idx = r.sample_indices_norepl(48)
    want = torch.cat([r.f_rewards[t, idx[16 * t:16 * t + 16], 0]
                      for t in range(3)])
    assert torch.equal(rew, want)


@pytest.mark.gpu
def test_captured_update_draws_without_replacement():
    from distributed_sac_amd.algo import SACEngine
    torch.manual_seed(0)
    cfg = SACConfig()
    cfg.variant, cfg.device = "mtsac", "cuda"
    cfg.state_dim, cfg.action_dim, cfg.num_tasks = 12, DA, 3
    cfg.actor_hidden_dim = cfg.critic_hidden_dim = [64, 64]
    cfg.batch_size = 48
    eng = SACEngine(cfg, "cuda:0", precision="bf16")
    r = ShardedReplay(3 * CAP, 3, cfg.mtobs_dim, DA, device="cuda:0",
                      sampling=NOREPL)
    fill(r, SIZES)
    for t in range(3):     # valid one-hot task suffix
        r.f_states[t, :, -3:] = 0
        r.f_states[t, :, -3 + t] = 1
        r.f_next_states[t, :, -3:] = r.f_states[t, :, -3:]
    r.f_rewards.mul_(1e-3)
    if not eng._use_krng:   # DSAC_KRNG=0: no counter, a clear error
        with pytest.raises(RuntimeError, match="attach_rng"):
            eng.capture(r, 48, warmup_iters=1)
        return
    eng.capture(r, 48, warmup_iters=1)
    torch.cuda.synchronize()
    c0 = int(eng._rng_ctr)
    for _ in range(2):
        m = eng.graphed_update()
    torch.cuda.synchronize()
    for k, v in m.items():
        assert float(v) == float(v) and abs(float(v)) != float("inf"), k
    assert int(eng._rng_ctr) == c0 + 2
    draw = torch_ref.replay_sample_indices_norepl
    assert not torch.equal(draw(r.sizes_dev, 48, 3, c0),
                           draw(r.sizes_dev, 48, 3, c0 + 1))


@pytest.mark.gpu
def test_learner_eager_gpu_path_has_the_counter():
    """Without a captured graph nobody calls capture(); the learner itself
    attaches the engine's counter, so the kernel path still works."""
    from distributed_sac_amd.workers.learner import Learner
    from distributed_sac_amd.workers.orchestrator import _actor_numel
    from distributed_sac_amd.workers.param_server import ParamSnapshot
    from tests.test_engine import small_cfg
    cfg = small_cfg("mtsac")
    cfg.buffer_size = 4 * CAP
    lr = Learner(cfg, "cuda:0", ParamSnapshot(_actor_numel(cfg)),
                 queue.Queue(), use_graph=False, precision="bf16",
                 sampling=NOREPL)
    assert lr.replay.sampling == NOREPL
    fill(lr.replay, (CAP, 40, 17, 33))
    lr.replay.f_rewards.mul_(1e-3)
    for f in (lr.replay.f_states, lr.replay.f_next_states):
        f[:, :, -4:] = torch.eye(4, device="cuda")[:, None, :]
    if not lr.engine._use_krng:   # DSAC_KRNG=0: no counter, a clear error
        with pytest.raises(RuntimeError, match="attach_rng"):
            lr.train_step()
        return
    c0 = int(lr.engine._rng_ctr)
    for _ in range(2):
        lr.train_step()
    torch.cuda.synchronize()
    assert int(lr.engine._rng_ctr) == c0 + 2
    assert lr.grad_steps == 2
    assert bool(torch.isfinite(lr.engine.actor_group.flat_data).all())


@pytest.mark.gpu
def test_default_mode_untouched():
    from distributed_sac_amd import ops
    r = make_replay(device="cuda", sampling="replace")
    ctr = torch.tensor([12345], dtype=torch.int64, device="cuda")
    r.attach_rng(ctr)
    got = r.sample(48, graph_safe=True)
    want = ops.native().replay_sample(
        r.f_states, r.f_actions, r.f_rewards, r.f_next_states, r.f_dones,
        r.sizes_dev, torch.empty(0, device="cuda"), 48, ctr)
    for name, w in zip(("states", "actions", "rewards", "next_states",
                        "dones"), want):
        assert torch.equal(got[name], w), name
