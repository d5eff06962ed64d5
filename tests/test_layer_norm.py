"""LayerNorm critics: the torch_ref contract against F.layer_norm, the mode's
switches, checkpoints, the unsupported paths, and the bf16 manual GPU update
against a float64 evaluation of the same update."""

import copy

import pytest
import torch
import torch.nn.functional as F

from distributed_sac_amd.algo import SACEngine, create_engine
from distributed_sac_amd.config import SACConfig, load_variant
from distributed_sac_amd.ops import torch_ref as R
from tests.test_engine import make_batch, small_cfg
from tests.test_pcgrad import stratified_batch


def ln_cfg(variant, on=True):
    cfg = small_cfg(variant)
    cfg.critic_layer_norm = on
    return cfg


def test_torch_ref_matches_layer_norm():
    g = torch.Generator().manual_seed(0)
    dims = [11, 24, 40, 3]
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa
    ws = [mk(n, k).requires_grad_() for k, n in zip(dims[:-1], dims[1:])]
    bs = [(mk(n) + 50.0).requires_grad_() for n in dims[1:]]
    gs = [(mk(n) * 0.3 + 1).requires_grad_() for n in dims[1:-1]]
    be = [mk(n).requires_grad_() for n in dims[1:-1]]
    x = mk(9, dims[0]).requires_grad_()
    leaves = [x, *ws, *bs, *gs, *be]
    h = x
    for i in range(2):
        h = F.relu(F.layer_norm(F.linear(h, ws[i], bs[i]), (dims[i + 1],),
                                gs[i], be[i], 1e-5))
    want = F.linear(h, ws[2], bs[2])
    got = R.ln_mlp_forward(x, ws, bs, gs, be)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    dy = mk(9, 3)
    for a, b in zip(torch.autograd.grad(got, leaves, dy),
                    torch.autograd.grad(want, leaves, dy)):
        assert torch.allclose(a, b, rtol=1e-10, atol=1e-10)


def test_switches(monkeypatch):
    assert not any(load_variant(v).critic_layer_norm_choice
                   for v in ("sac", "vsac", "mtsac", "care"))
    assert SACConfig.from_dict(
        {"critic_layer_norm": True}).critic_layer_norm_choice
    monkeypatch.setenv("DSAC_CRITIC_LN", "1")
    assert SACConfig().critic_layer_norm_choice
    assert not SACConfig.from_dict(
        {"critic_layer_norm": False}).critic_layer_norm_choice
    monkeypatch.setenv("DSAC_CRITIC_LN", "yes")
    for bad in (SACConfig.from_dict,
                lambda d: SACConfig().critic_layer_norm_choice):
        with pytest.raises(ValueError, match="(?i)critic_l"):
            bad({"critic_layer_norm": 1})


@pytest.mark.parametrize("variant", ["sac", "mtsac"])
def test_mode_off_is_the_parent(variant):
    torch.manual_seed(0)
    plain = SACEngine(small_cfg(variant), "cpu")
    torch.manual_seed(0)
    off = SACEngine(ln_cfg(variant, on=False), "cpu")
    a, b = plain.checkpoint_state(), off.checkpoint_state()
    name = "local_critic_1" if variant == "sac" else "local_critic"
    assert list(a[name]) == list(b[name])
    assert not off.cfg.critic_layer_norm_choice
    assert off.critic_group.numel == plain.critic_group.numel
    eps = [torch.randn(16, off.cfg.action_dim) for _ in range(2)]
    plain._eps_queue, off._eps_queue = copy.deepcopy(eps), copy.deepcopy(eps)
    assert plain.update(make_batch(off.cfg)) == off.update(make_batch(off.cfg))
    assert torch.equal(plain.critic_group.flat_data, off.critic_group.flat_data)


@pytest.mark.parametrize("variant", ["sac", "mtsac"])
def test_cpu_update_and_checkpoint(variant):
    torch.manual_seed(0)
    cfg = ln_cfg(variant)
    e = SACEngine(cfg, "cpu")
    plain = SACEngine(small_cfg(variant), "cpu")
    hidden = sum(cfg.critic_hidden_dim)
    assert e.critic_group.numel == plain.critic_group.numel + 4 * hidden
    lo = plain.critic_group.numel          # gamma and beta follow the Linears
    before = e.critic_group.flat_data.clone()
    m = e.update(make_batch(cfg))
    assert all(v == v for v in m.values())
    assert (e.critic_group.flat_data[lo:] != before[lo:]).any()
    assert not torch.equal(e.target_group.flat_data[lo:], before[lo:])

    ckpt = e.checkpoint_state()
    e2 = SACEngine(cfg, "cpu")
    e2.load_checkpoint_state(ckpt)
    eps = [torch.randn(cfg.batch_size, cfg.action_dim) for _ in range(2)]
    e._eps_queue, e2._eps_queue = copy.deepcopy(eps), copy.deepcopy(eps)
    assert e.update(make_batch(cfg, seed=1)) == \
        e2.update(make_batch(cfg, seed=1))
    with pytest.raises(ValueError, match="with LayerNorm.*without"):
        plain.load_checkpoint_state(ckpt)
    with pytest.raises(ValueError, match="without LayerNorm.*with"):
        e2.load_checkpoint_state(plain.checkpoint_state())


def test_unsupported_care():
    care = load_variant("care")
    care.critic_layer_norm = True
    with pytest.raises(NotImplementedError, match="critic_layer_norm: CARE"):
        create_engine(care, "cpu")


@pytest.mark.gpu
def test_unsupported_fp32_gpu():
    with pytest.raises(NotImplementedError, match="critic_layer_norm: .*fp32"):
        SACEngine(ln_cfg("sac"), "cuda:0", precision="fp32")


def _rnd(t, on):
    """t rounded to bf16 (straight through for autograd) where ``on``."""
    return t + (t.detach().bfloat16().double() - t.detach()) if on else t


def _chain(x, ws, bs, gam, bet, on):
    """float64 MLP chain, LayerNorm where ``gam`` is given.  ``on`` puts a
    bf16 rounding at each rounding point of the chain kernels: the input,
    the weights and h forward, the gradient at every linear output (dz, dy)
    backward."""
    h = _rnd(x, on)
    for i, (w, b) in enumerate(zip(ws, bs)):
        z = F.linear(h, _rnd(w, on), b)
        if on and z.requires_grad:
            z.register_hook(lambda g: g.bfloat16().double())
        if i == len(ws) - 1:
            return z
        if gam:
            d = z - z.mean(-1, keepdim=True)
            # h comes from the unrounded xhat; its bf16 copy serves the
            # backward only
            xh = d * torch.rsqrt((d * d).mean(-1, keepdim=True) + 1e-5)
            z = xh * gam[i] + bet[i]
        h = _rnd(torch.relu(z), on)


def _twin(e, x, on, target=False):
    pairs = e._critic_layer_pairs(target)
    norms = e._critic_norm_pairs(target)
    return [_chain(x, [p[q].weight for p in pairs], [p[q].bias for p in pairs],
                   [n[q] for n in norms], [n[2 + q] for n in norms], on)
            for q in (0, 1)]


def _flat_grad(loss, group):
    return torch.cat([g.reshape(-1) for g in
                      torch.autograd.grad(loss, group.params)])


@pytest.mark.gpu
@pytest.mark.parametrize("pcgrad", [False, True])
def test_engine_bf16_update(pcgrad, monkeypatch):
    """One manual bf16 update (mtsac, 64-wide, B = 64, T = 4) against float64
    from the same bf16-representable weights, batch and eps.

    Gradients (critic flat gradient, actor flat gradient through the
    post-step critic; with pcgrad the sums of the per-task arena rows): the
    reference is the float64 autograd evaluation with a bf16 rounding at each
    of the kernels' rounding points (``_chain(on=True)``).  What that leaves
    between kernel and reference (fp32 sums, a rounding that falls the other
    way, xhat's rounding inside the LayerNorm derivative) cannot be derived
    end to end, so the bound is measured on the reference alone: E = the
    change of the float64 gradient when those roundings are switched off,
    i.e. what the bf16 format itself does to this gradient (a few percent
    at B = 64: a rounding that moves a pre-activation across zero flips a
    ReLU mask).  Per parameter tensor p, with E'_p = max(E_p, |ref_p| E /
    |ref|) (E_p of a one-element tensor can vanish by chance):
    |got_p - ref_p| <= E'_p / 4 + 2 * 2^-8 |ref_p|.  The quarter: only
    roundings and masks that fall differently in fp32 and float64 count, a
    small share of all of them; 2 * 2^-8: the backward reads the
    bf16 xhat twice (dgamma, and xhat mean(g xhat) in dz), the reference
    the unrounded one.  Figures measured on the MI355X:
    profiles/layer_norm.md.

    Updated critic and target parameters: Adam's step and Polyak applied in
    float64 to the engine's own flat gradient.  fp32 bound on the step:
    1 - beta2^t in fp32 loses beta2 / (1 - beta2) = 999 ulps to cancellation
    (twice: bias correction and 1 - beta2), 1 - beta1^t likewise 9, 16 more
    for the remaining operations: (2 * 999 + 2 * 9 + 16) 2^-24 relative,
    plus 2 roundings of the parameter; the target, 4 roundings of it."""
    monkeypatch.setenv("DSAC_FUSE_TAIL", "0")    # leaves flat_grad folded
    torch.manual_seed(0)
    cfg = ln_cfg("mtsac")
    cfg.critic_hidden_dim = cfg.actor_hidden_dim = [64, 64]
    cfg.batch_size, cfg.pcgrad = 64, pcgrad
    ref_cfg = copy.deepcopy(cfg)
    ref_cfg.pcgrad = False
    ref = SACEngine(ref_cfg, "cpu")
    with torch.no_grad():    # LN parameters off their init, bf16 weights
        for grp in (ref.critic_group, ref.actor_group):
            grp.flat_data.add_(torch.randn(grp.numel) * 0.05)
            grp.flat_data.copy_(grp.flat_data.to(torch.bfloat16).float())
    ref.hard_copy_targets()
    gpu = SACEngine(cfg, "cuda:0", precision="bf16")
    gpu.load_checkpoint_state(ref.checkpoint_state())
    batch = stratified_batch(cfg)
    eps = [torch.randn(64, cfg.action_dim) for _ in range(2)]
    p0 = ref.critic_group.flat_data.double()
    gpu._eps_queue = [e.to("cuda") for e in eps]
    gpu.update({k: v.to("cuda") for k, v in batch.items()})
    cpu64 = lambda t: t.detach().cpu().double()   # noqa: E731

    # ---- updated critic and target from the engine's own gradient -------
    g = cpu64(gpu.critic_group.flat_grad)
    p1, t1 = cpu64(gpu.critic_group.flat_data), cpu64(gpu.target_group.flat_data)
    lr, u = cfg.lr_critic, 2.0 ** -24
    step = lr * g / (g.abs() + 1e-8)
    assert bool(((p1 - (p0 - step)).abs()
                 <= 2032 * u * step.abs() + 2 * u * p0.abs()).all())
    want_t = (1 - cfg.tau) * p0 + cfg.tau * p1
    assert bool(((t1 - want_t).abs() <= 4 * u * p0.abs().clamp(min=lr)).all())
    assert float(step.abs().max()) > 0.5 * lr

    # ---- the float64 evaluation -----------------------------------------
    for mod in (ref.actor, ref.local_critic, ref.target_critic):
        mod.double()
    A, T, k = cfg.action_dim, cfg.num_tasks, ref.actor.k
    b = {key: v.double() for key, v in batch.items()}
    s, s2 = b["states"], b["next_states"]
    la = ref.log_alpha.detach().double()
    alpha = (s[:, -T:] @ la).exp().unsqueeze(-1)
    w = R.task_weights(s[:, -T:], la.exp()).unsqueeze(-1)
    aw, ab = ref._actor_weights()

    def critic_grad(on):
        with torch.no_grad():
            o = _chain(s2, aw, ab, None, None, on)
            na, nlp, _ = R.squashed_gaussian(o[:, :A], o[:, A:],
                                             eps[0].double(), k)
            y = R.td_target(b["rewards"], b["dones"],
                            *_twin(ref, torch.cat([s2, na], -1), on, True),
                            nlp, alpha, ref.gamma, ref.reward_scale)
        q = _twin(ref, torch.cat([s, b["actions"]], -1), on)
        return _flat_grad(sum((w * (y - qi) ** 2).mean() for qi in q),
                          ref.critic_group)

    def actor_grad(on):
        o = _chain(s, aw, ab, None, None, on)
        a, lp, _ = R.squashed_gaussian(o[:, :A], o[:, A:], eps[1].double(), k)
        q = torch.min(*_twin(ref, torch.cat([s, a], -1), on))
        return _flat_grad((w * -(q - alpha * lp)).mean(), ref.actor_group)

    def check(got, fn, group, what):
        on, off = fn(True), fn(False)
        rel = float((on - off).norm() / off.norm())
        for p, o in zip(group.params, group.offsets):
            sl = slice(o, o + p.numel())
            err = float((got[sl] - on[sl]).norm())
            bound = 0.25 * max(float((on[sl] - off[sl]).norm()),
                               rel * float(off[sl].norm())) \
                + 2 * 2.0 ** -8 * float(on[sl].norm())
            print(what, tuple(p.shape), "err", err, "bound", bound,
                  "norm", float(off[sl].norm()))
            assert err <= bound, (what, tuple(p.shape))

    def got_grad(name, group):
        if not pcgrad:
            return cpu64(group.flat_grad)
        # the per-task arena rows add up to the plain gradient
        arena = next(v[0] for key, v in gpu._dw_arenas.items()
                     if key[0] == name and key[-1] == "per-task")
        return cpu64(arena[:, :group.numel]).sum(0)

    check(got_grad("critic", gpu.critic_group), critic_grad,
          ref.critic_group, "critic")
    with torch.no_grad():       # the actor step sees the post-step critic
        for p, o in zip(ref.critic_group.params, ref.critic_group.offsets):
            p.copy_(p1[o:o + p.numel()].view_as(p))
    check(got_grad("actor", gpu.actor_group), actor_grad, ref.actor_group,
          "actor")
