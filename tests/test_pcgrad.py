"""PCGrad off the GPU: the coefficient-space oracle and the CPU engine
against the literal vector-space algorithm of the paper in float64, the cfg
routes and the refused combinations."""

import math

import pytest
import torch

from distributed_sac_amd.algo import SACEngine, create_engine
from distributed_sac_amd.config import SACConfig, load_variant
from distributed_sac_amd.ops import functional as Fops
from distributed_sac_amd.ops import torch_ref as R
from tests.test_engine import make_batch, small_cfg


def make_grads(T, P, seed):
    """fp32 ``[T, P]``: g_t = s_t sqrt(P) 0.6 u + noise, u a unit vector,
    s_t = -1 for t % 3 == 1, else 1 — cosines of about +-0.26."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(P, generator=g, dtype=torch.float64)
    u /= u.norm()
    s = torch.tensor([-1.0 if t % 3 == 1 else 1.0 for t in range(T)],
                     dtype=torch.float64)
    noise = torch.randn(T, P, generator=g, dtype=torch.float64)
    return (s[:, None] * math.sqrt(P) * 0.6 * u + noise).float()


def literal_pcgrad(g, orders):
    """Algorithm 1 of the paper on ``g [T, P]`` in float64: the summed
    result, the projection count, the smallest |cosine| of a visited dot."""
    g = g.double()
    total, projected, min_cos = torch.zeros_like(g[0]), 0, float("inf")
    for i in range(g.shape[0]):
        gi = g[i].clone()
        for j in orders[i].tolist():
            d = gi @ g[j]
            min_cos = min(min_cos, float(d.abs() / (gi.norm() * g[j].norm())))
            if d < 0:
                gi -= d / (g[j] @ g[j]) * g[j]
                projected += 1
        total += gi
    return total, projected, min_cos


@pytest.mark.parametrize("T", [2, 3, 10, 16])
def test_oracle_matches_literal_algorithm(T):
    g = make_grads(T, 333, seed=T).double()
    orders = R.pcgrad_orders(T, 12345 + T, 0)
    assert sorted(orders[0].tolist()) == list(range(1, T))
    w, _, projected = R.pcgrad_weights(g @ g.T, orders, full=True)
    ref, ref_projected, _ = literal_pcgrad(g, orders)
    assert projected == ref_projected and projected >= T * (T - 1) // 3
    # float64 throughout: a few hundred roundings of 2^-53
    assert torch.allclose(R.pcgrad_fold(g, w), ref, rtol=0,
                          atol=1e-12 * float(ref.abs().max()))
    # no negative dot product: nothing is projected, the plain sum
    w1 = R.pcgrad_weights(g.abs() @ g.abs().T, orders)
    assert torch.equal(w1, torch.ones(T, dtype=torch.float64))


def pcgrad_cfg(T=3, B=12):
    cfg = small_cfg("mtsac")
    cfg.num_tasks, cfg.batch_size, cfg.pcgrad = T, B, True
    return cfg


def stratified_batch(cfg, seed=0):
    T, B = cfg.num_tasks, cfg.batch_size
    batch = make_batch(cfg, B, seed)
    oh = torch.nn.functional.one_hot(torch.arange(B) // (B // T), T).float()
    batch["states"][:, -T:] = oh
    batch["next_states"][:, -T:] = oh
    return batch


def _literal_step(ref, name, rows, group, opt, ctr):
    T = ref.num_tasks
    g = torch.stack([torch.cat([x.reshape(-1) for x in torch.autograd.grad(
        part, group.params, retain_graph=True)])
        for part in rows.reshape(T, -1).sum(dim=1)])
    total, projected, _ = literal_pcgrad(
        g, R.pcgrad_orders(T, ctr, R.PCGRAD_GROUPS[name]))
    group.flat_grad.copy_(total.float())
    opt.step()
    return projected


def test_cpu_update_matches_literal_algorithm():
    torch.manual_seed(0)
    cfg = pcgrad_cfg()
    e = SACEngine(cfg, "cpu")
    off = pcgrad_cfg()
    off.pcgrad = False
    ref = SACEngine(off, "cpu")
    ref.load_checkpoint_state(e.checkpoint_state())
    ref.hard_copy_targets()
    batch = stratified_batch(cfg)
    eps = [torch.randn(cfg.batch_size, cfg.action_dim) for _ in range(2)]
    e._eps_queue = [x.clone() for x in eps]
    ref._eps_queue = [x.clone() for x in eps]
    m = e.update(batch)

    # by hand: per-task autograd gradients, the literal algorithm, Adam
    st, ns = batch["states"], batch["next_states"]
    alpha = ref._per_sample_alpha(st)
    coeff = ref._row_coeff(st)
    ctr = int(torch.initial_seed()) & 0x7FFFFFFF
    with torch.no_grad():
        na, nlp, _ = ref._sample(ns)
        y = Fops.td_target(batch["rewards"], batch["dones"],
                           *ref._target_q(ns, na), nlp, alpha, ref.gamma,
                           ref.reward_scale)
    q1, q2 = ref.local_critic(st, batch["actions"])
    rows = coeff * ((y - q1) ** 2 + (y - q2) ** 2).reshape(-1)
    pc = _literal_step(ref, "critic", rows, ref.critic_group,
                       ref.critic_optimizer, ctr)
    sa, lp, _ = ref._sample(st)
    rows = coeff * -(torch.min(*ref.local_critic(st, sa))
                     - alpha * lp).reshape(-1)
    pa = _literal_step(ref, "actor", rows, ref.actor_group,
                       ref.actor_optimizer, ctr + 1)
    assert pc + pa > 0, "the case must project something"
    assert m["pcgrad_conflicts_critic"] == pytest.approx(pc / 6)
    assert m["pcgrad_conflicts_actor"] == pytest.approx(pa / 6)
    for ge, gr in ((e.critic_group, ref.critic_group),
                   (e.actor_group, ref.actor_group)):
        assert torch.allclose(ge.flat_data, gr.flat_data, atol=2e-6)

    # rows that are not laid out task by task are refused
    bad = stratified_batch(cfg)
    bad["states"][:, -3:] = bad["states"][:, -3:].flip(0)
    with pytest.raises(ValueError, match="task by task"):
        e.update_tensors(bad)


def test_cfg_routes(monkeypatch):
    assert not any(load_variant(v).pcgrad_choice
                   for v in ("mtsac", "care", "sac"))
    assert SACConfig.from_dict({"pcgrad": True}).pcgrad_choice
    monkeypatch.setenv("DSAC_PCGRAD", "1")
    assert SACConfig().pcgrad_choice
    assert not SACConfig.from_dict({"pcgrad": False}).pcgrad_choice
    monkeypatch.setenv("DSAC_PCGRAD", "yes")
    for bad in (SACConfig.from_dict, lambda d: SACConfig().pcgrad_choice):
        with pytest.raises(ValueError, match="(?i)pcgrad"):
            bad({"pcgrad": 1})


def test_refused_combinations():
    care, sac = load_variant("care"), small_cfg("sac")
    care.pcgrad = sac.pcgrad = True
    e = SACEngine(pcgrad_cfg(T=3, B=16), "cpu")
    for name, call in (
            ("CAREEngine", lambda: create_engine(care, "cpu")),
            ("num_tasks", lambda: SACEngine(pcgrad_cfg(T=17, B=34), "cpu")),
            ("num_tasks", lambda: SACEngine(sac, "cpu")),
            ("B % T", lambda: e.update_tensors(make_batch(e.cfg, 16))),
            ("data-parallel", lambda: SACEngine(pcgrad_cfg(), "cpu")
             .attach_ddp(type("Group", (), {"enabled": True})()))):
        with pytest.raises(NotImplementedError, match=name):
            call()
