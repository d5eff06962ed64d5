"""Opt-in gradient-norm clipping with a non-finite guard (max_grad_norm).

Only the sum of squares is toleranced: its summation order (docs/KERNELS.md
"Gradient-norm clipping") has a longest chain of L = ceil(n / 65536) + 18
dependent fp32 additions, so it agrees with a float64 sum of the same
squares to a relative (L + 2) * 2**-24.  norm and coef follow from it by
formula and everything downstream of coef is compared bit for bit.
"""

import copy
import glob
import math
import os
import queue
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from distributed_sac_amd.algo import CAREEngine, SACEngine
from distributed_sac_amd.config import (CANONICAL_CFGS, SACConfig, cfg_read,
                                        load_variant)
from distributed_sac_amd.ops import torch_ref
from distributed_sac_amd.ops.flat import FlatParams, FusedAdam
from tests.test_engine import make_batch, small_cfg

INF = float("inf")
SLOTS = 256                     # blocks (= partial slots) per range
LR, B1, B2, EPS = 3e-4, 0.9, 0.999, 1e-8


def chain_len(n: int) -> int:
    """Longest chain of dependent fp32 additions of the kernel's order:
    per-thread grid-stride accumulation, 6 wave steps, 3 adds over the four
    wave partials, then the re-sum of the slots: 3 adds per lane and 6
    wave steps."""
    return -(-n // (SLOTS * 256)) + 6 + 3 + 3 + 6


def sumsq_bound(n: int) -> float:
    return (chain_len(n) + 2) * 2.0 ** -24


def f32(x):
    return torch.tensor(x, dtype=torch.float32)


def sqrt_f32(s: torch.Tensor) -> torch.Tensor:
    """Correctly rounded fp32 square root (through float64: exact for
    sqrt; torch's own fp32 CPU sqrt is off by an ulp now and then)."""
    return f32(math.sqrt(float(s)))


def coef_of(norm: torch.Tensor, c: float) -> torch.Tensor:
    """min(1, c / (norm + 1e-6)) in IEEE fp32 (clip_grad_norm_'s formula)."""
    n = np.float32(float(norm))
    with np.errstate(over="ignore"):
        q = np.float32(c) / (n + np.float32(1e-6))
    return f32(float(min(np.float32(1.0), q)))


# ---------------------------------------------------------------------------
# CPU: plumbing
# ---------------------------------------------------------------------------

def test_cfg_key_round_trip_and_absent_by_default(monkeypatch):
    monkeypatch.delenv("DSAC_MAX_GRAD_NORM", raising=False)
    assert SACConfig().max_grad_norm is None
    c = SACConfig.from_dict({"max_grad_norm": 0.5})
    assert c.max_grad_norm == 0.5 and c.raw["max_grad_norm"] == 0.5
    assert c.max_grad_norm_choice == 0.5
    assert SACConfig.from_dict({"max_grad_norm": INF}).max_grad_norm == INF
    assert SACConfig.from_dict({"max_grad_norm": 3}).max_grad_norm == 3.0
    for variant in CANONICAL_CFGS:
        c = load_variant(variant)
        assert c.max_grad_norm is None and c.max_grad_norm_choice is None
        assert "max_grad_norm" not in c.raw
    ref_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                           "golden", "reference_cfg")
    paths = sorted(glob.glob(os.path.join(ref_dir, "*.json")))
    assert len(paths) == 5
    for path in paths:
        c = SACConfig.from_file(path)
        assert c.max_grad_norm is None and "max_grad_norm" not in c.raw
        assert c.raw == cfg_read(path)


@pytest.mark.parametrize("bad", [0, -1.0, float("nan"), True, False, "big",
                                 None, [1.0]])
def test_cfg_validation(bad):
    with pytest.raises(ValueError, match="max_grad_norm"):
        SACConfig.from_dict({"max_grad_norm": bad})
    if bad is not None:
        with pytest.raises(ValueError, match="max_grad_norm"):
            SACEngine(small_cfg("sac"), "cpu", max_grad_norm=bad)


def _thresholds(engine):
    return [o.max_grad_norm for o in (engine.critic_optimizer,
                                      engine.actor_optimizer,
                                      engine.log_alpha_optimizer)]


def test_env_default(monkeypatch):
    cfg = small_cfg("sac")
    monkeypatch.delenv("DSAC_MAX_GRAD_NORM", raising=False)
    assert _thresholds(SACEngine(cfg, "cpu")) == [None, None, None]
    monkeypatch.setenv("DSAC_MAX_GRAD_NORM", "0.25")
    assert _thresholds(SACEngine(cfg, "cpu")) == [0.25, 0.25, INF]
    # the cfg and the argument each beat the process-wide default
    cfg2 = copy.deepcopy(cfg)
    cfg2.max_grad_norm = 2.0
    assert _thresholds(SACEngine(cfg2, "cpu")) == [2.0, 2.0, INF]
    assert _thresholds(SACEngine(cfg2, "cpu", max_grad_norm=7.0)) \
        == [7.0, 7.0, INF]
    monkeypatch.setenv("DSAC_MAX_GRAD_NORM", "inf")
    assert _thresholds(SACEngine(cfg, "cpu")) == [INF, INF, INF]
    for bad in ("-1", "0", "nan", "lots"):
        monkeypatch.setenv("DSAC_MAX_GRAD_NORM", bad)
        with pytest.raises(ValueError, match="DSAC_MAX_GRAD_NORM|max_grad"):
            SACEngine(cfg, "cpu")


def test_launch_flag(monkeypatch, capsys):
    from distributed_sac_amd import launch
    from distributed_sac_amd.workers import orchestrator
    seen = {}

    class Stub:
        def __init__(self, cfg, **kw):
            seen.update(kw)

        def run(self, **kw):
            return {}

    monkeypatch.setattr(orchestrator, "DistributedTrainer", Stub)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["launch", "--variant", "sac",
                                      "--device", "cpu",
                                      "--max-grad-norm", "0.5"])
    launch.main()
    assert seen["max_grad_norm"] == 0.5
    monkeypatch.setattr(sys, "argv", ["launch", "--variant", "sac",
                                      "--device", "cpu"])
    launch.main()
    assert seen["max_grad_norm"] is None
    capsys.readouterr()


def test_learner_and_trainer_pass_it_through(monkeypatch):
    from distributed_sac_amd.workers.learner import Learner
    from distributed_sac_amd.workers.orchestrator import _actor_numel
    from distributed_sac_amd.workers.param_server import ParamSnapshot
    from distributed_sac_amd.workers.trainer import Trainer
    monkeypatch.delenv("DSAC_MAX_GRAD_NORM", raising=False)
    cfg = small_cfg("mtsac")
    cfg.buffer_size = 4 * 64
    cfg.max_grad_norm = 1.5

    def learner(c, **kw):
        return Learner(c, "cpu", ParamSnapshot(_actor_numel(c)),
                       queue.Queue(), use_graph=False, **kw)

    assert _thresholds(learner(cfg).engine) == [1.5, 1.5, INF]
    assert _thresholds(learner(cfg, max_grad_norm=4.0).engine) \
        == [4.0, 4.0, INF]
    plain = small_cfg("mtsac")
    plain.buffer_size = 4 * 64
    assert _thresholds(learner(plain).engine) == [None, None, None]
    assert _thresholds(Trainer(cfg, "cpu").engine) == [1.5, 1.5, INF]
    assert _thresholds(Trainer(plain, "cpu", max_grad_norm=0.5).engine) \
        == [0.5, 0.5, INF]


# ---------------------------------------------------------------------------
# CPU: Adam oracle, fallback
# ---------------------------------------------------------------------------

def _oracle_grads(shapes, norms, seed=0):
    """One gradient set per entry of ``norms``, scaled to that L2 norm."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for want in norms:
        gs = [torch.randn(*s, generator=g) for s in shapes]
        tot = math.sqrt(sum(float((x.double() ** 2).sum()) for x in gs))
        out.append([x * (want / tot) for x in gs])
    return out


def test_fused_adam_matches_torch_adam_with_clip_grad_norm():
    shapes = [(7, 5), (5,), (3, 3)]
    c = 1.0
    torch.manual_seed(0)
    ps = [nn.Parameter(torch.randn(*s)) for s in shapes]
    rs = [nn.Parameter(p.detach().clone()) for p in ps]
    group = FlatParams(ps)
    opt = FusedAdam(group, lr=1e-2, max_grad_norm=c)
    ref = torch.optim.Adam(rs, lr=1e-2)
    # well above, just above, just below, well below, above again
    norms = [50.0, 1.001, 0.999, 0.1, 3.0]
    for want, grads in zip(norms, _oracle_grads(shapes, norms)):
        for p, r, g in zip(ps, rs, grads):
            p.grad.copy_(g)
            r.grad = g.clone()
        before = group.flat_grad.clone()
        tn = torch.nn.utils.clip_grad_norm_(rs, c)
        ref.step()
        opt.step()
        assert torch.equal(group.flat_grad, before), "flat grad was scaled"
        assert float(opt.grad_norm) == pytest.approx(float(tn), rel=1e-6)
        assert float(opt.grad_norm) == pytest.approx(want, rel=1e-5)
        assert torch.equal(opt.clip_coef, coef_of(opt.grad_norm, c))
        assert (float(opt.clip_coef) < 1.0) == (want > c)
        for p, r in zip(ps, rs):
            torch.testing.assert_close(p.data, r.data, rtol=1e-6, atol=1e-7)
    assert int(opt.grad_skips) == 0 and opt.step_count == len(norms)


def test_fused_adam_off_has_no_clip_state():
    opt = FusedAdam(FlatParams([nn.Parameter(torch.ones(4))]), lr=1e-3)
    assert opt.max_grad_norm is None
    assert opt.grad_norm is None and opt.clip_coef is None
    assert opt.grad_skips is None


def _two_opts(device, betas2, c, seed=3):
    g = torch.Generator().manual_seed(seed)
    opts = []
    for k, n in enumerate((37, 5)):
        p = nn.Parameter(torch.randn(n, generator=g).to(device))
        grp = FlatParams([p])
        grp.flat_grad.copy_(torch.randn(n, generator=g) * 4)
        opts.append(FusedAdam(grp, lr=1e-2,
                              betas=(0.9, 0.999 if k == 0 else betas2),
                              max_grad_norm=c))
    return opts


def _check_fallback(device):
    c = 0.5
    many = _two_opts(device, 0.9, c)        # mismatched betas: unfused loop
    single = _two_opts(device, 0.9, c)
    unclipped = _two_opts(device, 0.9, None)
    FusedAdam.step_many(many)
    FusedAdam.step_many(unclipped)
    for o in single:
        o.step()
    for a, b, u in zip(many, single, unclipped):
        assert float(a.clip_coef) < 1.0
        assert torch.equal(a.clip_coef.cpu(), coef_of(a.grad_norm, c))
        assert torch.equal(a.group.flat_data, b.group.flat_data)
        assert torch.equal(a.exp_avg, b.exp_avg)
        assert torch.equal(a.exp_avg_sq, b.exp_avg_sq)
        assert not torch.equal(a.exp_avg, u.exp_avg)
        # m after the first step is (1 - b1) * coef * g
        want = (1.0 - 0.9) * (a.group.flat_grad * a.clip_coef)
        torch.testing.assert_close(a.exp_avg, want, rtol=1e-6, atol=1e-9)


def test_step_many_fallback_clips():
    _check_fallback("cpu")


# ---------------------------------------------------------------------------
# CPU: engine parity against the reference math + clip_grad_norm_
# ---------------------------------------------------------------------------

class _ClippedAdamSteps:
    """Patches torch.optim.Adam.step — the optimizer of the reference side
    of the existing reference-math tests — to call clip_grad_norm_ on the
    optimizer's own parameters first: at ``c`` (a callable of the step
    record, so that the first step can set it), guard-only for the
    one-parameter alpha optimizer."""

    def __init__(self, monkeypatch, threshold):
        self.calls = []         # (n_params, norm, max_norm)
        real = torch.optim.Adam.step
        outer = self

        def step(opt, *a, **kw):
            params = [p for g in opt.param_groups for p in g["params"]]
            c = INF if len(params) == 1 else threshold(outer.calls)
            if c is None:
                norm = torch.nn.utils.clip_grad_norm_(params, INF)
            else:
                norm = torch.nn.utils.clip_grad_norm_(params, c)
            outer.calls.append((len(params), float(norm), c))
            return real(opt, *a, **kw)

        monkeypatch.setattr(torch.optim.Adam, "step", step)


def _first_critic_norm(run, monkeypatch):
    """The reference side's own first-step critic norm, from an unclipped
    run of the same test (the critic optimizer steps first)."""
    with monkeypatch.context() as mp:
        rec = _ClippedAdamSteps(mp, lambda calls: None)
        run()
    assert rec.calls[0][0] > 1
    return rec.calls[0][1]


@pytest.mark.parametrize("variant", ["sac", "mtsac"])
def test_engine_matches_reference_math_with_clipping(variant, monkeypatch):
    """tests/test_engine.py::test_update_matches_reference_math (3 updates,
    atol=2e-6) with clip_grad_norm_ per optimizer on its reference side and
    max_grad_norm on the engine."""
    import tests.test_engine as te
    monkeypatch.delenv("DSAC_MAX_GRAD_NORM", raising=False)
    c = 0.5 * _first_critic_norm(
        lambda: te.test_update_matches_reference_math(variant), monkeypatch)
    rec = _ClippedAdamSteps(monkeypatch, lambda calls: c)
    engines = []

    def engine(cfg, device):
        engines.append(SACEngine(cfg, device, max_grad_norm=c))
        return engines[-1]

    monkeypatch.setattr(te, "SACEngine", engine)
    te.test_update_matches_reference_math(variant)
    assert len(engines) == 1 and engines[0].max_grad_norm == c
    critic = rec.calls[0::3]
    assert len(critic) == 3
    for n_params, norm, thr in critic:      # it really clipped, every step
        assert n_params > 1 and thr == c and norm > c
    assert float(engines[0].critic_optimizer.clip_coef) < 1.0
    assert float(engines[0].critic_optimizer.grad_norm) == \
        pytest.approx(critic[-1][1], rel=1e-5)
    assert int(engines[0].critic_optimizer.grad_skips) == 0


@pytest.mark.parametrize("modified", [True, False])
def test_care_matches_reference_math_with_clipping(modified, tmp_path,
                                                   monkeypatch):
    """tests/test_care.py::test_care_update_matches_reference_math at its
    own tolerance, clip_grad_norm_ per optimizer (critic, actor and, for
    original CARE, the context encoder) on the reference side."""
    import tests.test_care as tc
    monkeypatch.delenv("DSAC_MAX_GRAD_NORM", raising=False)
    c = 0.5 * _first_critic_norm(
        lambda: tc.test_care_update_matches_reference_math(tmp_path,
                                                           modified),
        monkeypatch)
    rec = _ClippedAdamSteps(monkeypatch, lambda calls: c)
    engines = []

    def engine(cfg, device):
        engines.append(CAREEngine(cfg, device, max_grad_norm=c))
        return engines[-1]

    monkeypatch.setattr(tc, "CAREEngine", engine)
    tc.test_care_update_matches_reference_math(tmp_path, modified)
    per_step = 3 if modified else 4
    assert len(rec.calls) == 3 * per_step
    for n_params, norm, thr in rec.calls[0::per_step]:
        assert n_params > 1 and thr == c and norm > c
    e = engines[0]
    assert (e.context_encoder_optimizer is not None) == (not modified)
    if not modified:
        assert e.context_encoder_optimizer.max_grad_norm == c
        assert float(e.context_encoder_optimizer.grad_norm) == \
            pytest.approx(rec.calls[-1][1], rel=1e-5)
    assert int(e.critic_optimizer.grad_skips) == 0


# ---------------------------------------------------------------------------
# CPU: bit-identity with inf, skip, metric keys
# ---------------------------------------------------------------------------

BASE_KEYS = {"critic_loss", "actor_loss", "alpha_loss", "entropy"}


def _make_engine(kind, tmp_path, device="cpu", **kw):
    torch.manual_seed(0)
    if kind in ("care", "care_original"):
        from tests.test_care import care_cfg
        cfg = care_cfg(tmp_path, modified=kind == "care")
        return cfg, CAREEngine(cfg, device, **kw)
    cfg = small_cfg(kind)
    return cfg, SACEngine(cfg, device, **kw)


def _opts(engine):
    out = {"critic": engine.critic_optimizer, "actor": engine.actor_optimizer,
           "alpha": engine.log_alpha_optimizer}
    ctx = getattr(engine, "context_encoder_optimizer", None)
    if ctx is not None:
        out["context"] = ctx
    return out


def _state(engine):
    """Every parameter, both moments and the targets, as clones."""
    out = {"target": engine.target_group.flat_data.clone()}
    for name, o in _opts(engine).items():
        out[name + ".p"] = o.group.flat_data.clone()
        out[name + ".m"] = o.exp_avg.clone()
        out[name + ".v"] = o.exp_avg_sq.clone()
    return out


def _eps(cfg, step):
    g = torch.Generator().manual_seed(900 + step)
    return [torch.randn(cfg.batch_size, cfg.action_dim, generator=g)
            for _ in range(2)]


def _run_updates(engine, cfg, batches):
    keys = None
    for step, b in enumerate(batches):
        engine._eps_queue = _eps(cfg, step)
        keys = set(engine.update({k: v.clone() for k, v in b.items()}))
    return keys


@pytest.mark.parametrize("kind", ["sac", "mtsac", "care", "care_original"])
def test_inf_threshold_is_bit_identical_to_off(kind, tmp_path, monkeypatch):
    monkeypatch.delenv("DSAC_MAX_GRAD_NORM", raising=False)
    cfg, off = _make_engine(kind, tmp_path)
    _, on = _make_engine(kind, tmp_path, max_grad_norm=INF)
    batches = [make_batch(cfg, cfg.batch_size, seed=s) for s in range(3)]
    keys_off = _run_updates(off, cfg, batches)
    keys_on = _run_updates(on, cfg, batches)
    assert keys_off == BASE_KEYS
    extra = {"critic_grad_norm", "actor_grad_norm", "grad_skips"}
    if kind == "care_original":
        extra.add("context_grad_norm")
    assert keys_on == BASE_KEYS | extra
    s_off, s_on = _state(off), _state(on)
    assert s_off.keys() == s_on.keys()
    for k in s_off:
        assert torch.equal(s_off[k], s_on[k]), k
    for o in _opts(on).values():
        assert float(o.clip_coef) == 1.0 and float(o.grad_norm) > 0.0
        assert int(o.grad_skips) == 0


@pytest.mark.parametrize("kind", ["sac", "mtsac", "care", "care_original"])
def test_nan_reward_skips_the_critic_step(kind, tmp_path, monkeypatch):
    """A NaN reward makes the critic gradient (and original CARE's context
    gradient, which comes from the critic loss) non-finite: those groups
    keep their bits and each bumps the skip counter once; the actor and
    alpha gradients of the same update are finite and step as usual."""
    monkeypatch.delenv("DSAC_MAX_GRAD_NORM", raising=False)
    cfg, e = _make_engine(kind, tmp_path, max_grad_norm=1.0)
    _run_updates(e, cfg, [make_batch(cfg, cfg.batch_size, seed=0)])
    before = _state(e)
    steps = e.critic_optimizer.step_count
    bad = make_batch(cfg, cfg.batch_size, seed=1)
    bad["rewards"][3] = float("nan")
    e._eps_queue = _eps(cfg, 1)
    m = e.update(bad)
    after = _state(e)
    skipped = ["critic"] + (["context"] if kind == "care_original" else [])
    for name in skipped:
        for part in (".p", ".m", ".v"):
            assert torch.equal(before[name + part], after[name + part]), name
        assert not math.isfinite(float(_opts(e)[name].grad_norm))
        assert float(_opts(e)[name].clip_coef) == 0.0
    assert m["grad_skips"] == len(skipped)
    assert int(e.critic_optimizer.grad_skips) == len(skipped)  # one counter
    assert not math.isfinite(m["critic_grad_norm"])
    # bias correction counts attempted steps
    assert e.critic_optimizer.step_count == steps + 1
    for name in ("actor", "alpha"):
        assert not torch.equal(before[name + ".p"], after[name + ".p"])
        assert bool(torch.isfinite(after[name + ".p"]).all())
    assert math.isfinite(m["actor_grad_norm"])
    # a following clean batch updates normally
    e._eps_queue = _eps(cfg, 2)
    m = e.update(make_batch(cfg, cfg.batch_size, seed=2))
    final = _state(e)
    assert m["grad_skips"] == len(skipped)
    for k, v in final.items():
        assert bool(torch.isfinite(v).all()), k
    for name in skipped:
        assert not torch.equal(final[name + ".p"], after[name + ".p"])
    assert math.isfinite(m["critic_grad_norm"])


# ---------------------------------------------------------------------------
# CPU: data parallel (gloo, world 2)
# ---------------------------------------------------------------------------

def _dp_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["WORLD_SIZE"] = str(world)
    os.environ["RANK"] = str(rank)
    os.environ["LOCAL_RANK"] = str(rank)
    os.environ.pop("DSAC_MAX_GRAD_NORM", None)
    torch.set_num_threads(1)
    torch.manual_seed(100 + rank)
    from distributed_sac_amd.parallel import DataParallelGroup
    cfg = small_cfg("mtsac")
    engine = SACEngine(cfg, "cpu", max_grad_norm=0.05)
    engine.attach_ddp(DataParallelGroup(backend="gloo"))
    # the critic gradient of the last update before and after its
    # all-reduce (on this path the actor backward later adds to the buffer)
    local = {}
    real = engine.ddp.allreduce_grad_

    def spy(t):
        mine = t.data_ptr() == engine.critic_group.flat_grad.data_ptr()
        if mine:
            local["g"] = t.clone()
        out = real(t)
        if mine:
            local["avg"] = t.clone()
        return out

    engine.ddp.allreduce_grad_ = spy
    for step in range(3):
        batch = make_batch(cfg, seed=1000 * rank + step)    # different data
        engine._eps_queue = [
            torch.randn(cfg.batch_size, cfg.action_dim,
                        generator=torch.Generator().manual_seed(step * 7 + k))
            for k in range(2)]
        m = engine.update(batch)
    q.put((rank,
           engine.actor_group.flat_data.numpy().copy(),
           engine.critic_group.flat_data.numpy().copy(),
           engine.log_alpha.detach().numpy().copy(),
           local["avg"].numpy().copy(),
           local["g"].numpy().copy(),
           m["critic_grad_norm"], float(engine.critic_optimizer.clip_coef),
           float(engine.actor_optimizer.clip_coef)))
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_dp_replicas_stay_identical_with_clipping():
    import numpy as np
    import torch.multiprocessing as mp
    from tests.test_ddp import _free_port
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(2):
        r = q.get()
        res[r[0]] = r[1:]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    a, b = res[0], res[1]
    for k in range(4):      # actor, critic, log_alpha, averaged critic grad
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a[4], b[4])       # the local gradients differ
    assert np.allclose(a[3], 0.5 * (a[4] + b[4]), atol=1e-7)
    # the reported norm is the averaged gradient's, the same on both ranks
    want = math.sqrt(float((a[3].astype(np.float64) ** 2).sum()))
    n = a[3].size
    assert a[5] == b[5] and a[6] == b[6] and a[7] == b[7]
    assert abs(a[5] - want) <= want * sumsq_bound(n)
    assert a[6] < 1.0 and a[7] < 1.0            # both groups clipped


# ---------------------------------------------------------------------------
# GPU: the sum-of-squares kernel
# ---------------------------------------------------------------------------

def _ext():
    from distributed_sac_amd.ops import native
    return native()


def _slot_tree(slots: torch.Tensor) -> torch.Tensor:
    """The Adam kernel's re-sum of one range's 256 slots: lane l adds slots
    l, l+64, l+128, l+192 in that order, then six xor-butterfly steps (32,
    16, ... 1); every lane ends with the same bits."""
    q = slots.detach().cpu().float().reshape(4, 64)
    v = ((q[0] + q[1]) + q[2]) + q[3]
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[lane ^ off]
    assert bool((v == v[0]).all())
    return v[0]


def _check_sumsq(s: torch.Tensor, g: torch.Tensor):
    want = float((g.detach().cpu().double() ** 2).sum())
    got = float(s)
    print(f"n={g.numel()} s={got!r} f64={want!r} "
          f"rel={abs(got - want) / want:.3e} bound={sumsq_bound(g.numel()):.3e}")
    assert abs(got - want) <= want * sumsq_bound(g.numel())


@pytest.mark.gpu
@pytest.mark.parametrize("arena_S", [None, 1, 7])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000, 65539])
def test_sumsq_single_range(n, arena_S):
    ext = _ext()
    gen = torch.Generator(device="cuda").manual_seed(13 * n + (arena_S or 0))
    slots = torch.full((3 * SLOTS,), float("nan"), device="cuda")
    if arena_S is None:
        g = torch.randn(n, device="cuda", generator=gen) * 3
        g_in = g.clone()
        ext.grad_sumsq_([g], slots)
        assert torch.equal(g, g_in)                 # only read
        again = torch.zeros_like(slots)
        ext.grad_sumsq_([g], again)
    else:
        # one spare row that must not be summed
        arena = torch.randn(arena_S + 1, n, device="cuda", generator=gen)
        g_ref = torch.full((n,), 9.0, device="cuda")
        g = torch.full((n,), -9.0, device="cuda")
        ext.reduce_arena(arena, g_ref, arena_S)
        ext.grad_sumsq_([g], slots, arena, arena_S)
        assert torch.equal(g.view(torch.int32), g_ref.view(torch.int32))
        again = torch.zeros_like(slots)
        ext.grad_sumsq_([torch.empty_like(g)], again, arena, arena_S)
    assert torch.equal(slots[:SLOTS].view(torch.int32),
                       again[:SLOTS].view(torch.int32))
    assert bool(torch.isnan(slots[SLOTS:]).all())   # other ranges untouched
    # blocks past the data wrote an exact zero
    used = min(SLOTS, -(-n // 256))
    assert bool((slots[used:SLOTS] == 0).all())
    _check_sumsq(_slot_tree(slots[:SLOTS]), g)


@pytest.mark.gpu
def test_sumsq_three_unaligned_ranges():
    ext = _ext()
    gen = torch.Generator(device="cuda").manual_seed(5)
    sizes, offs = (1000, 10, 300), (1, 1003, 1017)
    buf = torch.randn(1400, device="cuda", generator=gen)
    gs = [buf[o:o + n] for o, n in zip(offs, sizes)]
    assert all(g.data_ptr() % 16 != 0 for g in gs)
    keep = buf.clone()
    slots = torch.zeros(3 * SLOTS, device="cuda")
    ext.grad_sumsq_(gs, slots)
    again = torch.ones(3 * SLOTS, device="cuda")
    ext.grad_sumsq_(gs, again)
    assert torch.equal(slots.view(torch.int32), again.view(torch.int32))
    assert torch.equal(buf, keep)
    for r, g in enumerate(gs):
        _check_sumsq(_slot_tree(slots[r * SLOTS:(r + 1) * SLOTS]), g)
    # with an arena on range 0 the other ranges are unchanged
    arena = torch.randn(3, 1000, device="cuda", generator=gen)
    ref0 = torch.empty(1000, device="cuda")
    ext.reduce_arena(arena, ref0, 3)
    folded = torch.zeros(3 * SLOTS, device="cuda")
    ext.grad_sumsq_(gs, folded, arena, 3)
    assert torch.equal(gs[0], ref0)
    assert torch.equal(buf[1001:], keep[1001:]) and buf[0] == keep[0]
    assert torch.equal(folded[SLOTS:], slots[SLOTS:])
    _check_sumsq(_slot_tree(folded[:SLOTS]), ref0)


# ---------------------------------------------------------------------------
# GPU: Adam with coef, skip
# ---------------------------------------------------------------------------

def _adam_state(n, gen, with_mirror=True):
    p = torch.randn(n, device="cuda", generator=gen)
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    st = torch.zeros(3, device="cuda")
    mir = (torch.zeros(n, device="cuda", dtype=torch.bfloat16)
           if with_mirror else None)
    return [p, m, v, st, mir]


def _clone(state):
    return [t.clone() if t is not None else None for t in state]


def _multi_args(groups, grads):
    return ([g[0] for g in groups], list(grads), [g[1] for g in groups],
            [g[2] for g in groups], [g[3] for g in groups],
            [LR] * len(groups), B1, B2, EPS,
            [g[4] if g[4] is not None else torch.Tensor() for g in groups])


def _clip_extras(G, thresholds, shared_skips=False):
    slots = torch.zeros(3 * SLOTS, device="cuda")
    cs = [torch.zeros(3, device="cuda") for _ in range(G)]
    if shared_skips:
        sk = [torch.zeros(1, dtype=torch.int32, device="cuda")] * G
    else:
        sk = [torch.zeros(1, dtype=torch.int32, device="cuda")
              for _ in range(G)]
    return slots, list(thresholds), cs, sk


def _assert_groups_equal(new, ref):
    for gn, gr in zip(new, ref):
        for a, b in zip(gn, gr):
            if a is not None:
                if a.dtype == torch.float32:
                    a, b = a.view(torch.int32), b.view(torch.int32)
                assert torch.equal(a, b)


def _norm64(g):
    return math.sqrt(float((g.double() ** 2).sum()))


def _check_published(cs, slots, r, g, c):
    """{norm, coef, s}: s is the slot tree, norm and coef follow by formula."""
    norm, coef, s = cs.cpu()
    assert torch.equal(s, _slot_tree(slots[r * SLOTS:(r + 1) * SLOTS]))
    _check_sumsq(s, g)
    assert torch.equal(norm, sqrt_f32(s))
    assert torch.equal(coef, coef_of(norm, c))
    return coef


@pytest.mark.gpu
@pytest.mark.parametrize("clips", [True, False])
@pytest.mark.parametrize("mirror", [True, False])
@pytest.mark.parametrize("arena_S", [None, 7])
@pytest.mark.parametrize("n", [1, 257, 1000])
def test_adam_dev_with_coef(n, arena_S, mirror, clips):
    """One group (FusedAdam.step): bit-equal to adam_step_dev_ fed g * coef
    (a torch fp32 multiply), or fed g when the threshold is above the
    norm."""
    ext = _ext()
    gen = torch.Generator(device="cuda").manual_seed(31 * n + (arena_S or 0))
    ref = _adam_state(n, gen, mirror)
    new = _clone(ref)
    g_new = torch.full((n,), -9.0, device="cuda")
    for _ in range(2):              # two consecutive steps, own prologs
        if arena_S is None:
            g = torch.randn(n, device="cuda", generator=gen)
            g_new.copy_(g)
            arena_args = ()
        else:
            arena = torch.randn(arena_S + 1, n, device="cuda", generator=gen)
            g = torch.empty(n, device="cuda")
            ext.reduce_arena(arena, g, arena_S)
            arena_args = (arena, arena_S)
        c = _norm64(g) * (0.5 if clips else 2.0)
        slots, cl, cs, sk = _clip_extras(1, [c])
        p, m, v, st, mir = new
        ext.adam_step_clip_([p], [g_new], [m], [v], [st], [LR], B1, B2, EPS,
                            [mir if mirror else torch.Tensor()], slots, cl,
                            cs, sk, None, 0, *arena_args)
        assert torch.equal(g_new.view(torch.int32), g.view(torch.int32))
        coef = _check_published(cs[0], slots, 0, g, c)
        assert (float(coef) < 1.0) == clips
        fed = g * coef.cuda() if clips else g
        p, m, v, st, mir = ref
        ext.adam_step_dev_(p, fed, m, v, st, LR, B1, B2, EPS, mir, 0)
        _assert_groups_equal([new], [ref])
        assert int(sk[0]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("clips", [True, False])
@pytest.mark.parametrize("mirrors", [True, False])
@pytest.mark.parametrize("tail", [False, True])
def test_adam_multi_with_coef(tail, mirrors, clips):
    """Three groups on their own norms (the third guarded only); with
    ``tail`` the first comes as a split-K arena and a Polyak range rides
    along, as in the engine's last launch."""
    ext = _ext()
    gen = torch.Generator(device="cuda").manual_seed(77 + tail + 2 * mirrors)
    sizes = (1000, 300, 10)
    ref = [_adam_state(n, gen, mirrors and n != 10) for n in sizes]
    new = [_clone(g) for g in ref]
    NP, tau = 513, 0.005
    src = torch.randn(NP, device="cuda", generator=gen)
    t_ref = torch.randn(NP, device="cuda", generator=gen)
    t_new = t_ref.clone()
    pm_ref = (torch.zeros(NP, device="cuda", dtype=torch.bfloat16)
              if mirrors else None)
    pm_new = pm_ref.clone() if mirrors else None
    # unaligned gradient slices of one buffer, as the actor+alpha arena
    buf = torch.zeros(1 + sum(sizes), device="cuda")
    g_new, off = [], 1
    for n in sizes:
        g_new.append(buf[off:off + n])
        off += n
    for _ in range(2):
        gs = [torch.randn(n, device="cuda", generator=gen) * 2 for n in sizes]
        extra = ()
        if tail:
            arena = torch.randn(4, sizes[0], device="cuda", generator=gen)
            ext.reduce_arena(arena, gs[0], 3)
            extra = (arena, 3, t_new, src, tau, pm_new)
        for dst, g in zip(g_new, gs):
            dst.copy_(g)
        if tail:
            g_new[0].fill_(-9.0)
        scale = 0.5 if clips else 2.0
        thr = [_norm64(gs[0]) * scale, _norm64(gs[1]) * scale, INF]
        slots, cl, cs, sk = _clip_extras(3, thr)
        ext.adam_step_clip_(*_multi_args(new, g_new), slots, cl, cs, sk,
                            None, 0, *extra)
        fed = []
        for r, (g, c) in enumerate(zip(gs, thr)):
            assert torch.equal(g_new[r].view(torch.int32),
                               g.view(torch.int32))
            coef = _check_published(cs[r], slots, r, g, c)
            assert (float(coef) < 1.0) == (clips and r < 2)
            fed.append(g * coef.cuda() if float(coef) < 1.0 else g)
        ext.adam_step_multi_(*_multi_args(ref, fed))
        _assert_groups_equal(new, ref)
        if tail:
            ext.polyak_(t_ref, src, tau, pm_ref)
            assert torch.equal(t_new, t_ref)
            if mirrors:
                assert torch.equal(pm_new, pm_ref)
        assert all(int(s) == 0 for s in sk)


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("case", ["inf", "nan", "both"])
def test_adam_multi_skips_non_finite_group(case, shared):
    """Three groups + Polyak range; an inf / a NaN in one group's gradient
    leaves that group's p, m, v and mirror alone and bumps its counter;
    the rest of the launch equals the unguarded kernel."""
    ext = _ext()
    gen = torch.Generator(device="cuda").manual_seed(len(case) + 5 * shared)
    sizes = (700, 300, 10)
    ref = [_adam_state(n, gen) for n in sizes]
    new = [_clone(g) for g in ref]
    NP, tau = 513, 0.005
    src = torch.randn(NP, device="cuda", generator=gen)
    t_ref = torch.randn(NP, device="cuda", generator=gen)
    t_new = t_ref.clone()
    pm_ref = torch.zeros(NP, device="cuda", dtype=torch.bfloat16)
    pm_new = pm_ref.clone()
    bad = {"inf": {1: INF}, "nan": {0: float("nan")},
           "both": {0: -INF, 2: float("nan")}}[case]
    slots, cl, cs, sk = _clip_extras(3, [INF, INF, INF], shared)
    # a first step gives every group non-trivial moments and mirrors
    gs = [torch.randn(n, device="cuda", generator=gen) for n in sizes]
    ext.adam_step_clip_(*_multi_args(new, gs), slots, cl, cs, sk)
    ext.adam_step_multi_(*_multi_args(ref, gs))
    _assert_groups_equal(new, ref)
    for step in range(2):
        gs = [torch.randn(n, device="cuda", generator=gen) for n in sizes]
        for r, val in bad.items():
            gs[r][sizes[r] // 2] = val
        keep = [_clone(g) for g in new]
        g_in = [g.clone() for g in gs]
        ext.adam_step_clip_(*_multi_args(new, gs), slots, cl, cs, sk, None,
                            0, None, 0, t_new, src, tau, pm_new)
        ext.adam_step_multi_(*_multi_args(ref, gs), None, 0, None, 0,
                             t_ref, src, tau, pm_ref)
        for r in range(3):
            assert torch.equal(gs[r].view(torch.int32),
                               g_in[r].view(torch.int32))
            if r in bad:
                # p, m, v, mirror keep their bits; the step counter moved on
                for k in (0, 1, 2, 4):
                    assert torch.equal(new[r][k], keep[r][k])
                assert float(new[r][3][0]) == step + 2
                assert float(cs[r][1]) == 0.0
                assert not math.isfinite(float(cs[r][0]))
                # hand the unguarded side the kept state for the next step
                for k in (0, 1, 2, 4):
                    ref[r][k].copy_(keep[r][k])
            else:
                assert float(cs[r][1]) == 1.0
        _assert_groups_equal(new, ref)
        assert torch.equal(t_new, t_ref) and torch.equal(pm_new, pm_ref)
        if shared:
            assert int(sk[0]) == (step + 1) * len(bad)
        else:
            for r in range(3):
                assert int(sk[r]) == (step + 1 if r in bad else 0)


@pytest.mark.gpu
def test_step_many_fallback_clips_gpu():
    _check_fallback("cuda")


# ---------------------------------------------------------------------------
# GPU: engine, bf16 manual path, eager and captured
# ---------------------------------------------------------------------------

def _gpu_replay(cfg, nan_rewards=False):
    from distributed_sac_amd.replay import ShardedReplay
    dev = "cuda:0"
    g = torch.Generator().manual_seed(11)
    replay = ShardedReplay(4000, cfg.num_tasks, cfg.mtobs_dim,
                           cfg.action_dim, device=dev)
    for t in range(cfg.num_tasks):
        n = 256
        st = torch.randn(n, cfg.mtobs_dim, generator=g)
        st[:, -cfg.num_tasks:] = 0
        st[:, -cfg.num_tasks + t] = 1
        rew = torch.randn(n, 1, generator=g)
        if nan_rewards:
            rew.fill_(float("nan"))
        replay.shards[t].append(
            st.to(dev), (torch.rand(n, cfg.action_dim, generator=g) * 2
                         - 1).to(dev),
            rew.to(dev), st.clone().to(dev), torch.zeros(n, 1, device=dev))
    return replay


def _gpu_engine(c, monkeypatch):
    monkeypatch.delenv("DSAC_MAX_GRAD_NORM", raising=False)
    torch.manual_seed(0)
    cfg = small_cfg("mtsac")
    e = SACEngine(cfg, "cuda:0", precision="bf16", max_grad_norm=c)
    assert e._bf16 and e._use_krng
    return cfg, e


def _gpu_state(e):
    out = _state(e)
    out["critic.mirror"] = e.critic_optimizer.bf16_mirror.clone()
    out["actor.mirror"] = e.actor_optimizer.bf16_mirror.clone()
    return out


def _run_eager(c, monkeypatch, updates=3, nan_rewards=False):
    cfg, e = _gpu_engine(c, monkeypatch)
    replay = _gpu_replay(cfg, nan_rewards)
    replay.attach_rng(e._rng_ctr)
    for _ in range(updates):
        m = e.update_tensors(replay.sample(cfg.batch_size, graph_safe=True))
    torch.cuda.synchronize()
    return e, {k: v.detach().clone() for k, v in m.items()}


def _run_captured(c, monkeypatch, updates=3, nan_rewards=False):
    """One eager warm-up update, then ``updates - 1`` replays."""
    cfg, e = _gpu_engine(c, monkeypatch)
    replay = _gpu_replay(cfg, nan_rewards)
    e.capture(replay, cfg.batch_size, warmup_iters=1)
    for _ in range(updates - 1):
        m = e.graphed_update()
    torch.cuda.synchronize()
    return e, {k: v.detach().clone() for k, v in m.items()}


def _assert_same(a, b, keys=None):
    sa, sb = _gpu_state(a), _gpu_state(b)
    assert sa.keys() == sb.keys()
    for k in sa:
        if keys is None or k in keys:
            assert torch.equal(sa[k], sb[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("run", [_run_eager, _run_captured])
def test_engine_inf_is_bit_identical_to_off_gpu(run, monkeypatch):
    off, m_off = run(None, monkeypatch)
    on, m_on = run(INF, monkeypatch)
    assert set(m_off) == BASE_KEYS
    assert set(m_on) == BASE_KEYS | {"critic_grad_norm", "actor_grad_norm",
                                     "grad_skips"}
    _assert_same(off, on)
    for k in BASE_KEYS:
        assert torch.equal(m_off[k], m_on[k]), k
    assert int(m_on["grad_skips"]) == 0
    for o in _opts(on).values():
        assert float(o.clip_coef) == 1.0


@pytest.mark.gpu
def test_engine_clipped_capture_equals_eager_gpu(monkeypatch):
    c = 0.05
    eager, m_e = _run_eager(c, monkeypatch)
    cap, m_c = _run_captured(c, monkeypatch)
    _assert_same(eager, cap)
    assert m_e.keys() == m_c.keys()
    for k in m_e:
        assert torch.equal(m_e[k], m_c[k]), k
    # it clipped, and differs from the unclipped run
    off, _ = _run_eager(None, monkeypatch)
    assert not torch.equal(off.critic_group.flat_data,
                           eager.critic_group.flat_data)
    for e, m in ((eager, m_e), (cap, m_c)):
        for name, o in _opts(e).items():
            g = o.group.flat_grad       # the unclipped gradient
            norm, coef, s = o._clip_state.cpu()
            _check_sumsq(s, g)
            assert torch.equal(norm, sqrt_f32(s))
            assert torch.equal(coef, coef_of(norm, o.max_grad_norm))
            assert (float(coef) < 1.0) == (name != "alpha")
        assert torch.equal(m["critic_grad_norm"],
                           e.critic_optimizer.grad_norm)
        assert torch.equal(m["actor_grad_norm"], e.actor_optimizer.grad_norm)
        assert int(m["grad_skips"]) == 0


@pytest.mark.gpu
def test_engine_nan_rewards_skip_every_captured_replay_gpu(monkeypatch):
    cfg, e = _gpu_engine(1.0, monkeypatch)
    fresh = _gpu_state(e)
    replay = _gpu_replay(cfg, nan_rewards=True)
    e.capture(replay, cfg.batch_size, warmup_iters=1)
    torch.cuda.synchronize()
    assert int(e._grad_skips) == 1          # the eager warm-up update
    for k in range(3):
        m = e.graphed_update()
        torch.cuda.synchronize()
        assert int(m["grad_skips"]) == 2 + k
        assert not math.isfinite(float(m["critic_grad_norm"]))
        assert math.isfinite(float(m["actor_grad_norm"]))
    now = _gpu_state(e)
    for k in ("critic.p", "critic.m", "critic.v", "critic.mirror"):
        assert torch.equal(fresh[k], now[k]), k
    assert e.critic_optimizer.step_count == 4   # attempted steps
    for k in ("actor.p", "alpha.p"):
        assert not torch.equal(fresh[k], now[k])
        assert bool(torch.isfinite(now[k]).all()), k
