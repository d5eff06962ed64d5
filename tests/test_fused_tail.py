"""Fused small-kernel tail of the SAC update (DSAC_FUSE_TAIL).

Every fused kernel is checked against the composition of the kernels it
replaces, on the same inputs, with torch.equal: the fusions change no
arithmetic and no reduction order, so any mismatch is a bug.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

B_GRID = [1, 256, 257, 700]          # 1 block, exact block, 2 blocks, partial
WT_GRID = [(0, 1), (0, 10), (1, 10), (1, 32)]   # (use_w, T)


def _ext():
    from distributed_sac_amd.ops import native
    return native()


def _states(B, T, gen):
    s = torch.randn(B, 39 + T, device="cuda", generator=gen)
    idx = torch.randint(0, T, (B,), device="cuda", generator=gen)
    s[:, -T:] = torch.nn.functional.one_hot(idx, T).float()
    return s


def _randn(gen, *shape):
    return torch.randn(*shape, device="cuda", generator=gen)


@pytest.mark.parametrize("use_w,T", WT_GRID)
@pytest.mark.parametrize("B", B_GRID)
def test_critic_td_loss_matches_three_launches(B, use_w, T):
    ext = _ext()
    gen = torch.Generator(device="cuda").manual_seed(100 * B + T + use_w)
    states = _states(B, T, gen)
    r, q1t, q2t, q1, q2 = (_randn(gen, B, 1) for _ in range(5))
    nlp = _randn(gen, B, 1) * 3
    d = (torch.rand(B, 1, device="cuda", generator=gen) < 0.2).float()
    la = _randn(gen, T) * 0.3
    gamma, rs = 0.99, 1.5

    ws_ref = torch.zeros(256, device="cuda")
    y = ext.td_target_mt(r, d, q1t, q2t, nlp, states, la, T, gamma, rs)
    closs_ref = ext.critic_loss_fwd(q1, q2, y, states, la, T, use_w,
                                    ws_ref)[0]
    dq_ref = ext.critic_loss_bwd2(q1, q2, y, states, la, closs_ref, T,
                                  use_w)

    ws = torch.zeros(256, device="cuda")
    for _ in range(2):      # second call: the ticket has reset itself
        closs, dq = ext.critic_td_loss(r, d, q1t, q2t, nlp, q1, q2, states,
                                       la, T, use_w, gamma, rs, ws)
        assert float(ws[0]) == 0.0
        assert dq.shape == (2, B, 1) and dq.dtype == torch.bfloat16
        assert torch.equal(closs[:7], closs_ref[:7])
        assert torch.equal(dq, dq_ref)


@pytest.mark.parametrize("use_w,T", WT_GRID)
@pytest.mark.parametrize("B", B_GRID)
def test_actor_alpha_loss_fwd_bwd_matches_two_launches(B, use_w, T):
    ext = _ext()
    A, H_bar = 4, -4.0
    gen = torch.Generator(device="cuda").manual_seed(7 + 100 * B + T + use_w)
    states = _states(B, T, gen)
    aq1, aq2 = _randn(gen, B, 1), _randn(gen, B, 1)
    lp = _randn(gen, B, 1) * 3
    ls = _randn(gen, B, A)
    la = _randn(gen, T) * 0.3

    dla_ref = torch.full((T,), 7.5, device="cuda")
    al_ref = ext.actor_alpha_loss_fwd(aq1, aq2, lp, ls, states, la, T, use_w,
                                      H_bar, dla_ref,
                                      torch.zeros(256, device="cuda"))
    daq_ref, dlp_ref = ext.actor_alpha_loss_bwd2(
        aq1, aq2, lp, states, la, al_ref, dla_ref, T, use_w, H_bar,
        torch.zeros(2048, device="cuda"))

    # the critic loss over the same states / log_alpha finalizes the same
    # normalizer (closs[2]); the engine hands it over instead of having
    # every block recompute it
    y = _randn(gen, B, 1)
    closs = ext.critic_loss_fwd(aq1, aq2, y, states, la, T, use_w,
                                torch.zeros(256, device="cuda"))[0]
    assert torch.equal(closs[2], al_ref[1])

    ws = torch.zeros(1 + 32 * 4 + 32 * 32, device="cuda")
    for k in range(3):
        # garbage in the alpha flat grad: the kernel must overwrite it
        dla = torch.full((T,), float("nan") if k else -3.25, device="cuda")
        wsum = closs[2:3] if k == 2 else None
        al, daq, dlp = ext.actor_alpha_loss_fwd_bwd(
            aq1, aq2, lp, ls, states, la, dla, T, use_w, H_bar, ws, wsum)
        assert float(ws[0]) == 0.0
        assert torch.equal(al, al_ref)
        assert torch.equal(daq, daq_ref)
        assert torch.equal(dlp, dlp_ref)
        assert torch.equal(dla, dla_ref)
        # bit-equal including the sign of zero
        assert torch.equal(dla.view(torch.int32), dla_ref.view(torch.int32))


def _adam_state(n, gen, with_mirror=True):
    p = _randn(gen, n)
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    st = torch.zeros(3, device="cuda")
    mir = (torch.zeros(n, device="cuda", dtype=torch.bfloat16)
           if with_mirror else None)
    return [p, m, v, st, mir]


def _clone(state):
    return [t.clone() if t is not None else None for t in state]


LR, B1, B2, EPS = 3e-4, 0.9, 0.999, 1e-8


@pytest.mark.parametrize("S", [1, 7])
@pytest.mark.parametrize("n", [1, 255, 1000])
def test_adam_dev_folds_arena(n, S):
    ext = _ext()
    gen = torch.Generator(device="cuda").manual_seed(31 * n + S)
    ref = _adam_state(n, gen)
    new = _clone(ref)
    g_ref = torch.full((n,), 9.0, device="cuda")
    g_new = torch.full((n,), -9.0, device="cuda")
    for _ in range(2):          # two consecutive steps, each with its prolog
        arena = _randn(gen, S + 1, n)   # one spare row: only S are summed
        ext.reduce_arena(arena, g_ref, S)
        p, m, v, st, mir = ref
        ext.adam_step_dev_(p, g_ref, m, v, st, LR, B1, B2, EPS, mir, 0)
        p, m, v, st, mir = new
        ext.adam_step_dev_(p, g_new, m, v, st, LR, B1, B2, EPS, mir, 0,
                           arena, S)
        assert torch.equal(g_new, g_ref)
        for a, b in zip(new, ref):
            assert torch.equal(a, b)


def _multi_args(groups, grads):
    return ([g[0] for g in groups], list(grads), [g[1] for g in groups],
            [g[2] for g in groups], [g[3] for g in groups],
            [LR] * len(groups), B1, B2, EPS,
            [g[4] if g[4] is not None else torch.Tensor() for g in groups])


@pytest.mark.parametrize("S", [1, 7])
@pytest.mark.parametrize("n", [1, 255, 1000])
def test_adam_multi_folds_arena_of_group0(n, S):
    ext = _ext()
    gen = torch.Generator(device="cuda").manual_seed(17 * n + S)
    ref = [_adam_state(n, gen), _adam_state(10, gen, with_mirror=False)]
    new = [_clone(g) for g in ref]
    g0_ref = torch.full((n,), 9.0, device="cuda")
    g0_new = torch.full((n,), -9.0, device="cuda")
    for _ in range(2):
        arena = _randn(gen, S, n)
        g1 = _randn(gen, 10)            # the second group reads its flat grad
        ext.reduce_arena(arena, g0_ref, S)
        ext.adam_step_multi_(*_multi_args(ref, [g0_ref, g1]))
        ext.adam_step_multi_(*_multi_args(new, [g0_new, g1]), None, 0,
                             arena, S)
        assert torch.equal(g0_new, g0_ref)
        for gn, gr in zip(new, ref):
            for a, b in zip(gn, gr):
                if a is not None:
                    assert torch.equal(a, b)


@pytest.mark.parametrize("mirrors", [False, True])
def test_adam_multi_with_polyak_range(mirrors):
    ext = _ext()
    gen = torch.Generator(device="cuda").manual_seed(99 + mirrors)
    ref = [_adam_state(300, gen, with_mirror=mirrors),
           _adam_state(10, gen, with_mirror=False)]
    new = [_clone(g) for g in ref]
    NP, tau = 513, 0.005
    src = _randn(gen, NP)
    t_ref = _randn(gen, NP)
    t_new = t_ref.clone()
    pm_ref = (torch.zeros(NP, device="cuda", dtype=torch.bfloat16)
              if mirrors else None)
    pm_new = pm_ref.clone() if mirrors else None
    for _ in range(2):
        grads = [_randn(gen, 300), _randn(gen, 10)]
        ext.adam_step_multi_(*_multi_args(ref, grads))
        ext.polyak_(t_ref, src, tau, pm_ref)
        ext.adam_step_multi_(*_multi_args(new, grads), None, 0, None, 0,
                             t_new, src, tau, pm_new)
        assert torch.equal(t_new, t_ref)
        if mirrors:
            assert torch.equal(pm_new, pm_ref)
        for gn, gr in zip(new, ref):
            for a, b in zip(gn, gr):
                if a is not None:
                    assert torch.equal(a, b)


def test_step_many_fallback_keeps_rng_bump():
    """Mismatched betas force step_many's unfused loop: the RNG counter is
    still bumped exactly once, and each optimizer steps once."""
    import torch.nn as nn
    from distributed_sac_amd.ops.flat import FlatParams, FusedAdam
    opts = []
    for k in range(2):
        p = nn.Parameter(torch.ones(5, device="cuda"))
        grp = FlatParams([p])
        grp.flat_grad.fill_(0.5)
        opts.append(FusedAdam(grp, lr=1e-3, betas=(0.9, 0.999 - 0.1 * k)))
    ctr = torch.tensor([41], dtype=torch.int64, device="cuda")
    FusedAdam.step_many(opts, rng_bump=ctr)
    assert int(ctr) == 42
    assert [o.step_count for o in opts] == [1, 1]
    FusedAdam.step_many(opts, rng_bump=None, pre_prologed=False)
    assert int(ctr) == 42


def _engine_run(cfg, batches, fuse, monkeypatch):
    from distributed_sac_amd.algo import SACEngine
    monkeypatch.setenv("DSAC_FUSE_TAIL", "1" if fuse else "0")
    torch.manual_seed(0)
    engine = SACEngine(cfg, "cuda:0", precision="bf16")
    metrics = []
    for k in range(6):
        out = engine.update_tensors(batches[k % 3])
        metrics.append({n: v.clone() for n, v in out.items()})
    torch.cuda.synchronize()
    flats = [getattr(engine, n).flat_data.clone() for n in
             ("alpha_group", "actor_group", "critic_group", "target_group")]
    return flats, metrics


@pytest.mark.parametrize("shipped", [False, True])
def test_engine_fused_tail_matches_unfused(shipped, monkeypatch):
    import copy
    from distributed_sac_amd.config import load_variant
    from tests.test_engine import make_batch, small_cfg
    if shipped:
        cfg = load_variant("mtsac")
    else:
        cfg = copy.deepcopy(small_cfg("mtsac"))
    B = cfg.batch_size
    batches = [{k: v.cuda() for k, v in make_batch(cfg, B, seed=s).items()}
               for s in range(3)]
    flats1, met1 = _engine_run(cfg, batches, True, monkeypatch)
    flats0, met0 = _engine_run(cfg, batches, False, monkeypatch)
    for a, b in zip(flats1, flats0):
        assert torch.equal(a, b)
    for m1, m0 in zip(met1, met0):
        assert m1.keys() == m0.keys()
        for n in m1:
            assert torch.equal(m1[n], m0[n])
