"""PCGrad on the GPU: the Gram/solve and fold kernels against the float64
oracle, and the bf16 manual engine in PCGrad mode."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from distributed_sac_amd.ops import native  # noqa: E402
from distributed_sac_amd.ops import torch_ref as R  # noqa: E402
from tests.test_pcgrad import (literal_pcgrad, make_grads,  # noqa: E402
                               pcgrad_cfg, stratified_batch)

DEV = "cuda"
SHAPES = [(2, 0, 3), (3, 5, 333), (10, 0, 4096), (16, 64, 70001)]


def _arena(T, lo, n):
    """The gradients at [lo, lo + n) of [T, stride], NaN everywhere else."""
    stride = (lo + n + 3 + 3) // 4 * 4
    a = torch.full((T, stride), float("nan"))
    a[:, lo:lo + n] = make_grads(T, n, seed=1000 * T + n)
    return a.to(DEV)


def _solve(arena, T, lo, n, ctr, group=0):
    out = torch.zeros(532, device=DEV)
    native().pcgrad_gram_solve(
        arena, T, lo, n, torch.tensor([ctr], dtype=torch.int64, device=DEV),
        group, torch.zeros(1 + 128 * 256, device=DEV), out)
    return out.cpu()


def _parts(out, T):
    return (out[:T], out[16:20], out[20:276].view(16, 16),
            out[276:].view(16, 16)[:T, :T - 1].long())


@pytest.mark.parametrize("T,lo,n", SHAPES)
def test_gram(T, lo, n):
    arena = _arena(T, lo, n)
    out = _solve(arena, T, lo, n, 7)
    G = _parts(out, T)[2]
    g = arena[:, lo:lo + n].cpu()
    ref, tol = R.gemm_oracle(g, g, n=n)    # n fp32 additions in any order
    ratio = R.gemm_bound_ratio(G[:T, :T], ref, tol)
    print("worst err / bound:", float(ratio.max()))
    assert float(ratio.max()) <= 1.0
    assert not G[T:].any() and not G[:, T:].any()     # rows >= T stay zero
    assert torch.equal(out, _solve(arena, T, lo, n, 7)), "run to run"


def check_solve_and_fold(out, arena, flat, T, lo, n, ctr, group):
    """Solve and fold (``flat``) against float64 on the kernel's own G, w."""
    w, metrics, G, orders = _parts(out, T)
    want = R.pcgrad_orders(T, ctr, group)
    assert torch.equal(orders, want), "visiting orders, index for index"
    G64 = G[:T, :T].double()
    w64, a64, projected = R.pcgrad_weights(G64, want, full=True)
    assert metrics[:2].tolist() == [T * (T - 1), projected]
    assert float(metrics[3]) == pytest.approx(projected / (T * (T - 1)))
    # a_i[j] is written once, from a T-term fma chain, a division and a
    # subtraction: (T + 2) ulps on terms that sum to sum_k |a_i[k]| |G_kj| /
    # G_jj (the final a_i bounds the one at the step); errors of earlier
    # a_i[k] enter scaled by |G_kj| / G_jj.  w[t] adds T coefficients.
    absG, dg = G64.abs(), G64.diagonal()
    delta = torch.zeros(T, T, dtype=torch.float64)
    for i in range(T):
        for j in want[i].tolist():
            if a64[i, j] != 0:
                delta[i, j] = ((T + 2) * R.GEMM_ULP
                               * (a64[i].abs() @ absG[:, j])
                               + delta[i] @ absG[:, j]) / dg[j]
    tol_w = delta.sum(0) + T * R.GEMM_ULP * a64.abs().sum(0)
    err_w = (w.double() - w64).abs()
    print("w err", float(err_w.max()), "tol", float(tol_w.max()))
    assert bool((err_w <= tol_w).all())
    ref, tol = R.gemm_oracle(w[None, :], arena[:T, lo:lo + n].cpu().T, n=T)
    ratio = R.gemm_bound_ratio(flat[lo:lo + n].cpu()[None, :], ref, tol)
    assert float(ratio.max()) <= 1.0


@pytest.mark.parametrize("T,lo,n", SHAPES)
@pytest.mark.parametrize("ctr,group", [(12345, 0), (2 ** 31 - 3, 1)])
def test_weights_and_fold(T, lo, n, ctr, group):
    arena = _arena(T, lo, n)
    # no coin toss: in float64 every visited dot is well away from zero
    _, projected, min_cos = literal_pcgrad(
        arena[:, lo:lo + n].cpu(), R.pcgrad_orders(T, ctr, group))
    assert min_cos >= 1e-3
    assert T * (T - 1) / 3 <= projected <= T * (T - 1)
    out = _solve(arena, T, lo, n, ctr, group)
    flat = torch.full((arena.shape[1],), float("nan"), device=DEV)
    native().pcgrad_fold(arena, out.to(DEV), flat, T, lo, n)
    check_solve_and_fold(out, arena, flat, T, lo, n, ctr, group)
    keep = torch.ones_like(flat, dtype=torch.bool)
    keep[lo:lo + n] = False
    assert bool(torch.isnan(flat[keep]).all()), "a write outside the range"


def _engine(on):
    from distributed_sac_amd.algo import SACEngine
    cfg = pcgrad_cfg(T=3, B=96)
    cfg.actor_hidden_dim = cfg.critic_hidden_dim = [64, 64]
    cfg.pcgrad = on
    torch.manual_seed(0)
    return cfg, SACEngine(cfg, "cuda:0", precision="bf16")


def test_engine_gradients():
    T, B = 3, 96
    (cfg, e), (_, d) = _engine(True), _engine(False)
    batch = {k: v.to(DEV) for k, v in stratified_batch(cfg).items()}
    ctr = int(e._rng_ctr)
    for eng in (e, d):
        eng._manual_seg1(batch)
        eng._manual_seg2()
    torch.cuda.synchronize()
    # the Adam prolog of seg2 bumps the counter between the two groups
    for name, group, c in (("critic", e.critic_group, ctr),
                           ("actor", e.actor_group, ctr + 1)):
        arena = e._dw_arena(name, group.numel, B)[0]
        assert arena.shape == (T, (group.numel + 3) // 4 * 4)
        check_solve_and_fold(e._pcgrad_out[name].cpu(), arena,
                             group.flat_grad, T, 0, group.numel, c,
                             R.PCGRAD_GROUPS[name])
    # both splits add the same B exact bf16 products per element in fp32,
    # each within (B + S + 2) ulps of mag = sum |term|; mag is replaced by
    # its lower bound sum_t |arena_t|, which only tightens the check
    n = e.critic_group.numel
    arena = e._dw_arena("critic", n, B)[0][:, :n].double()
    diff = (arena.sum(0) - d.critic_group.flat_grad.double()).abs()
    bound = 2 * (B + T + 2) * R.GEMM_ULP * arena.abs().sum(0) + R.GEMM_FLOOR
    print("row sum vs default: worst err / bound",
          float((diff / bound).max()))
    assert bool((diff <= bound).all())


def _replay(cfg, T):
    from distributed_sac_amd.replay import ShardedReplay
    g = torch.Generator().manual_seed(5)
    rp = ShardedReplay(4000, T, cfg.mtobs_dim, cfg.action_dim,
                       device="cuda:0")
    for t in range(T):
        st = torch.randn(256, cfg.mtobs_dim, generator=g).to(DEV)
        st[:, -T:] = 0
        st[:, cfg.mtobs_dim - T + t] = 1
        rp.shards[t].append(
            st, torch.rand(256, cfg.action_dim, generator=g).to(DEV) * 2 - 1,
            torch.randn(256, 1, generator=g).to(DEV), st.clone(),
            torch.zeros(256, 1, device=DEV))
    return rp


def test_engine_captured_matches_eager():
    (cfg, cap), (_, eager) = _engine(True), _engine(True)
    replays = [_replay(cfg, 3), _replay(cfg, 3)]
    cap.capture(replays[0], cfg.batch_size)     # three eager warm-up updates
    for _ in range(3):
        m = cap.graphed_update()
        for k in ("pcgrad_conflicts_critic", "pcgrad_conflicts_actor"):
            assert 0.0 <= float(m[k]) <= 1.0
    replays[1].attach_rng(eager._rng_ctr)
    for _ in range(6):
        eager.update_tensors(replays[1].sample(cfg.batch_size,
                                               graph_safe=True))
    torch.cuda.synchronize()
    # fixed-order sums throughout: replays repeat eager bit for bit
    for name in ("critic", "actor"):
        assert torch.equal(cap._pcgrad_out[name], eager._pcgrad_out[name])
    assert torch.equal(cap.critic_group.flat_data,
                       eager.critic_group.flat_data)
    assert torch.equal(cap.actor_group.flat_data, eager.actor_group.flat_data)


@pytest.mark.parametrize("name,env,precision", [
    ("fp32 GPU path", None, None), ("DSAC_NO_MANUAL", "1", "bf16"),
    ("DSAC_KRNG", "0", "bf16")])
def test_refused_on_gpu(monkeypatch, name, env, precision):
    from distributed_sac_amd.algo import SACEngine
    if env is not None:
        monkeypatch.setenv(name, env)
    with pytest.raises(NotImplementedError, match=name):
        SACEngine(pcgrad_cfg(), "cuda:0", precision=precision)
