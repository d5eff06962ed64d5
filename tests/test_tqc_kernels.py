"""Truncated quantile critics on the GPU: the two loss kernels, the chain
kernels at a quantile head width and the bf16 engine, each against the
float64 ``torch_ref`` forward with ``torch.autograd`` on it, from the same
fp32 inputs."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from distributed_sac_amd.ops import torch_ref as R  # noqa: E402

DEV = "cuda"
GAMMA, RS = 0.99, 0.5


def _ext():
    from distributed_sac_amd import ops
    return ops.native()


def _rows(B, T, g):
    """states with a one-hot suffix, log_alpha, the task of each row."""
    states = torch.randn(B, 7 + T, generator=g)
    idx = torch.randint(0, T, (B,), generator=g)
    states[:, -T:] = torch.nn.functional.one_hot(idx, T).float()
    return states, torch.randn(T, generator=g) * 0.3, idx


def _coeff64(states, la, T, use_w):
    B = states.shape[0]
    if use_w:
        return R.task_weights(states[:, -T:].double(), la.double().exp()) / B
    return torch.full((B,), 1.0 / B, dtype=torch.float64)


@pytest.mark.parametrize("T,use_w", [(1, 0), (1, 1), (10, 0), (10, 1)])
@pytest.mark.parametrize("B", [1, 5, 67, 300])
@pytest.mark.parametrize("M,drop", [(1, 0), (5, 2), (25, 2), (32, 5)])
def test_tqc_critic_loss(M, drop, B, T, use_w):
    ext = _ext()
    g = torch.Generator().manual_seed(1000 * M + 10 * B + T + use_w)
    states, la, idx = _rows(B, T, g)
    base = torch.randn(B, 1, generator=g) * 2
    # atoms within about +-3 of each other: |u| straddles 1, both signs
    zt1, zt2, th1, th2 = (base + torch.randn(B, M, generator=g) * 1.5
                          for _ in range(4))
    zt2[:, 0] = zt1[:, 0]                      # ties across the networks
    if M > 1:
        zt1[:, 1] = zt1[:, 0]                  # and within one
    r = torch.randn(B, 1, generator=g)
    dn = (torch.rand(B, 1, generator=g) < 0.3).float()
    nlp = torch.randn(B, 1, generator=g)
    K = 2 * M - 2 * drop

    th64 = [t.double().requires_grad_(True) for t in (th1, th2)]
    y = R.tqc_target(r.double(), dn.double(), zt1.double(), zt2.double(),
                     nlp.double(), la.double().exp()[idx].unsqueeze(1),
                     GAMMA, RS, drop)
    c = _coeff64(states, la, T, use_w)
    l1, l2 = R.tqc_critic_loss(*th64, y, c)
    ref_d = torch.stack(torch.autograd.grad(l1 + l2, th64))
    amax = torch.stack([th1, th2]).double().abs().amax(dim=(0, 2))
    bound = 2.0 ** -8 * ref_d.abs() + (
        c / (M * K) * K * 2.0 ** -18
        * (1 + y.abs().amax(dim=1) + amax)).view(1, B, 1)

    ws = torch.zeros(1 + 2 * 1024, device=DEV)

    def run(z2):
        out = ext.tqc_critic_loss(
            r.to(DEV), dn.to(DEV), zt1.to(DEV), z2.to(DEV), nlp.to(DEV),
            th1.to(DEV), th2.to(DEV), states.to(DEV), la.to(DEV), T, use_w,
            GAMMA, RS, drop, ws)
        assert int(ws[:1].view(torch.int32)) == 0     # the ticket is reset
        return out[0].cpu(), out[1].float().cpu().double()

    closs, dth = run(zt2)
    err = (dth - ref_d).abs()
    print(f"max err/bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all())
    for got, ref in ((closs[0], l1), (closs[1], l2), (closs[6], l1 + l2)):
        assert abs(got.item() - ref.item()) <= 1e-4 * abs(ref.item())
    closs2, dth2 = run(zt2)
    assert torch.equal(closs[:7], closs2[:7]) and torch.equal(dth, dth2)

    if B > 1:   # one NaN target atom poisons its row, and only its row
        bad = B // 2
        z2 = zt2.clone()
        z2[bad, M // 2] = float("nan")
        closs, dth = run(z2)
        assert bool(dth[:, bad].isnan().all()) and bool(closs[6].isnan())
        keep = torch.arange(B) != bad
        assert bool(((dth - ref_d).abs() <= bound)[:, keep].all())


def test_tqc_critic_loss_limits():
    ext = _ext()
    ws = torch.zeros(1 + 2 * 1024, device=DEV)

    def run(B, M, drop):
        z, one = (torch.zeros(B, n, device=DEV) for n in (M, 1))
        ext.tqc_critic_loss(one, one, z, z, one, z, z,
                            torch.ones(B, 3, device=DEV),
                            torch.zeros(1, device=DEV), 1, 0, GAMMA, RS,
                            drop, ws)

    with pytest.raises(RuntimeError, match="B <= 8192"):
        run(8200, 2, 0)
    with pytest.raises(RuntimeError, match="drop"):
        run(8, 2, 2)
    with pytest.raises(RuntimeError, match="2M <= 64"):
        run(8, 33, 2)


@pytest.mark.parametrize("T,use_w", [(1, 0), (10, 1)])
@pytest.mark.parametrize("M", [1, 5, 25])
def test_tqc_actor_alpha_loss(M, T, use_w):
    ext = _ext()
    B, A = 300, 4
    H_bar = -float(A)
    g = torch.Generator().manual_seed(50 + M + T)
    states, la, idx = _rows(B, T, g)
    aq1, aq2 = (torch.randn(B, M, generator=g) for _ in range(2))
    lp, ls = torch.randn(B, 1, generator=g), torch.randn(B, A, generator=g)

    a64 = [t.double().requires_grad_(True) for t in (aq1, aq2)]
    lp64 = lp.double().requires_grad_(True)
    la64 = la.double().requires_grad_(True)
    la_g = la64[idx].unsqueeze(1)
    c = _coeff64(states, la, T, use_w).unsqueeze(1)
    pl = (c * -(R.tqc_q(*a64) - la_g.exp().detach() * lp64)).sum()
    al_loss = -(la_g * (lp64.detach() + H_bar)).mean()
    ent = R.entropy_from_log_std(ls.double())
    g1, g2, glp, gla = torch.autograd.grad(pl + al_loss, a64 + [lp64, la64])

    dla = torch.full((T,), 7.0, device=DEV)
    wsum = None
    if use_w:   # as the engine: the critic loss of the update finalized it
        wsum = torch.nn.functional.softmax(-la.exp(), 0)[idx].sum()
        wsum = wsum.reshape(1).to(DEV)
    al, daq, dlp = ext.tqc_actor_alpha_loss_fwd_bwd(
        aq1.to(DEV), aq2.to(DEV), lp.to(DEV), ls.to(DEV), states.to(DEV),
        la.to(DEV), dla, T, use_w, H_bar,
        torch.zeros(1 + 32 * 4 + 32 * 32, device=DEV), wsum)
    al = al.cpu().double()
    for got, ref in ((al[0], pl), (al[2], al_loss), (al[3], ent)):
        assert torch.allclose(got, ref.detach(), atol=1e-5, rtol=1e-4)
    assert torch.allclose(dlp.cpu().double(), glp, atol=1e-6, rtol=1e-4)
    assert torch.allclose(dla.cpu().double(), gla, atol=1e-6, rtol=1e-4)
    daq = daq.float().cpu().double()
    ref = torch.stack([g1, g2])
    assert daq.shape == ref.shape
    assert bool(((daq - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-7).all())


@pytest.mark.parametrize("chain", ["1", "0"])
def test_chain_kernels_at_quantile_head(chain, monkeypatch):
    """G = 2 with a 25-wide head.  Forward: layer by layer on the kernel's
    saved inputs, the bound of torch_ref.gemm_oracle.  input_grad and
    backward: the float64 backward from the saved activations, the same
    bound carried through the layers (a bf16 dy hands tol @ |W| on)."""
    from distributed_sac_amd.ops.chain import ManualChain, pack_chains
    from distributed_sac_amd.ops.flat import FlatParams
    monkeypatch.setenv("DSAC_CHAIN", chain)
    G, M, widths, lo = 2, 96, [21, 48, 40, 25], 17
    g = torch.Generator().manual_seed(3)
    ws = [torch.nn.Parameter((torch.randn(G, N, K, generator=g)
                              / K ** 0.5).to(DEV))
          for K, N in zip(widths[:-1], widths[1:])]
    bs = [torch.nn.Parameter(torch.randn(G, N, generator=g).to(DEV))
          for N in widths[1:]]
    group = FlatParams(ws + bs)
    w16 = [w.detach().to(torch.bfloat16) for w in ws]
    ch = ManualChain(w16, [b.detach() for b in bs], G=G, group=group,
                     w_params=ws, b_params=bs)
    pack_chains(_ext(), [(ch, True, True)])
    x1 = torch.randn(M, lo, generator=g).to(DEV)
    x2 = torch.randn(M, widths[0] - lo, generator=g).to(DEV)
    y, acts = ch.forward(x1, x2)
    L = len(ws)
    x = acts[0].reshape(1, M, -1).expand(G, M, -1)
    for li in range(L):
        got = y if li == L - 1 else acts[li + 1]
        ref, tol = R.gemm_oracle(x, w16[li], bs[li].detach(),
                                 relu=li < L - 1)
        assert bool(torch.isfinite(R.gemm_bound_ratio(got, ref, tol)).all())
        x = got

    dy = torch.randn(G, M, widths[-1], generator=g).to(DEV).to(torch.bfloat16)
    S, chunk = 2, 64
    arena = torch.zeros(S, group.numel, device=DEV)
    dsa = ch.input_grad(dy, acts, lo)
    ch.backward(dy, acts, arena, S, chunk)
    fold = arena.double().sum(0)
    ref, tol = dy.double(), torch.zeros_like(dy, dtype=torch.float64)
    ins = [acts[0].reshape(1, M, -1).expand(G, M, -1)] + list(acts[1:])
    for li in range(L - 1, -1, -1):
        # dW [G, N, K] = dy^T x over M rows in S partial sums; db likewise
        a = ins[li].double()
        for off, n_el, rhs in ((group.offsets[li], ws[li].numel(), a),
                               (group.offsets[L + li], bs[li].numel(),
                                torch.ones(G, M, 1, dtype=torch.float64,
                                           device=DEV))):
            want = ref.transpose(1, 2) @ rhs
            mag = ref.abs().transpose(1, 2) @ rhs.abs()
            t = tol.transpose(1, 2) @ rhs.abs()
            bound = t + (M + S + 2) * R.GEMM_ULP * (mag + t) + R.GEMM_FLOOR
            got = fold[off:off + n_el].view_as(want)
            assert bool(((got - want).abs() <= bound).all()), li
        w = w16[li].double()
        if li == 0:
            w = w[:, :, lo:]
        nref, mag, t = ref @ w, ref.abs() @ w.abs(), tol @ w.abs()
        ntol = t + (w.shape[1] + 2) * R.GEMM_ULP * (mag + t) + R.GEMM_FLOOR
        if li > 0:   # masked by the ReLU of the saved activation, then bf16
            mask = acts[li] != 0
            nref, ntol = nref * mask, ntol * mask
            ntol = ntol + R.BF16_ROUNDOFF * (nref.abs() + ntol)
        ref, tol = nref, ntol
    if chain == "0":   # the per-layer mode sums the groups, in bf16
        ref, tol = ref.sum(0), tol.sum(0) + R.GEMM_ULP * 3 * ref.abs().sum(0)
        tol = tol + R.BF16_ROUNDOFF * (ref.abs() + tol)
    assert dsa.shape == ref.shape
    assert bool(((dsa.double() - ref).abs() <= tol).all())


@pytest.mark.parametrize("variant", ["sac", "mtsac"])
def test_tqc_engine_bf16_tracks_cpu_and_captures(variant):
    from distributed_sac_amd.algo import SACEngine
    from distributed_sac_amd.replay import ShardedReplay
    from tests.test_engine import make_batch, small_cfg
    torch.manual_seed(0)
    cfg = small_cfg(variant)
    cfg.critic_quantiles, cfg.critic_quantiles_drop = 5, 1
    cpu = SACEngine(cfg, "cpu")
    gpu = SACEngine(cfg, "cuda:0", precision="bf16")
    gpu.load_checkpoint_state(cpu.checkpoint_state())
    gpu.hard_copy_targets()
    batch = make_batch(cfg)
    eps = [torch.randn(cfg.batch_size, cfg.action_dim) for _ in range(2)]
    cpu._eps_queue = [e.clone() for e in eps]
    gpu._eps_queue = [e.to(DEV) for e in eps]
    mc = cpu.update(batch)
    mg = gpu.update({k: v.to(DEV) for k, v in batch.items()})
    for k in ("critic_loss", "actor_loss"):
        print(k, mc[k], mg[k])
        assert abs(mc[k] - mg[k]) < 0.25 + 0.25 * abs(mc[k])

    T = gpu.num_tasks
    replay = ShardedReplay(4000, T, cfg.mtobs_dim, cfg.action_dim,
                           device="cuda:0")
    for t in range(T):
        st = torch.randn(256, cfg.mtobs_dim, device=DEV)
        if T > 1:
            st[:, -T:] = 0
            st[:, cfg.mtobs_dim - T + t] = 1
        replay.shards[t].append(
            st, torch.rand(256, cfg.action_dim, device=DEV) * 2 - 1,
            torch.randn(256, 1, device=DEV), st.clone(),
            torch.zeros(256, 1, device=DEV))
    gpu.capture(replay, cfg.batch_size)
    for _ in range(5):
        m = gpu.graphed_update()
        assert all(bool(torch.isfinite(v)) for v in m.values())


def test_tqc_unsupported_on_gpu(monkeypatch):
    from distributed_sac_amd.algo import SACEngine
    from tests.test_engine import small_cfg
    cfg = small_cfg("sac")
    cfg.critic_quantiles, cfg.critic_quantiles_drop = 5, 1
    with pytest.raises(NotImplementedError, match="quantile"):
        SACEngine(cfg, "cuda:0")                       # the fp32 GPU path
    monkeypatch.setenv("DSAC_NO_MANUAL", "1")
    with pytest.raises(NotImplementedError, match="quantile"):
        SACEngine(cfg, "cuda:0", precision="bf16")
