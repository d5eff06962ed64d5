"""k_f32_chain_dx / k_f32_chain_dwdb: the whole fp32 MLP backward in three
launches (DSAC_F32_CHAIN_BWD=1), against float64 bounds and against the
per-layer path.  Observed err / bound per shape: profiles/f32_chain_bwd.md."""

import functools

import pytest
import torch

from distributed_sac_amd.ops import functional as Fops
from distributed_sac_amd.ops import native, torch_ref
from tests.test_f32_chain import CAP, DEV, SHAPES, _int_net, _net

pytestmark = pytest.mark.gpu

CASES = [(s, M, G) for s in ("critic", "unaligned", "narrow", "cap_mid",
                             "one") for M in (1, 17, 33) for G in (1, 2)]


@functools.lru_cache(maxsize=None)
def _chain(shape, M, G):
    """(ws, acts, dy): a net, what its forward saves, a random dy."""
    x1, x2, ws, bs = _net(shape, M, G)
    y, acts = native().mlp_chain_fwd_f32(x1, x2, ws, bs, G, True)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(1))
    return ws, acts, dy.to(DEV)


def _worst(ratio, out, ref, tol):
    assert out.shape == ref.shape
    return float(ratio(out, ref, tol).max()) if out.numel() else 0.0


@pytest.mark.parametrize("shape,M,G,nan",
                         [(*c, False) for c in CASES]
                         + [("critic", 17, 2, True)])
def test_dx_walk_within_float64_bound(shape, M, G, nan):
    ws, acts, dy = _chain(shape, M, G)
    if nan:      # one NaN row: it spreads through that row and no other
        dy = dy.clone()
        dy[..., M // 2, :] = float("nan")
    ratio = torch_ref.bound_ratio if nan else torch_ref.gemm_bound_ratio
    L, c1, worst = len(ws), SHAPES[shape][0], 0.0
    for lo in (0, c1):
        dys, dx0 = native().mlp_chain_bwd_dx_f32(dy, ws, acts, G, lo)
        above = [*dys, dy]
        assert len(dys) == L - 1
        for l in range(L - 1, 0, -1):   # judged from the kernel's own dy_l
            ref, tol = torch_ref.gemm_oracle(
                above[l], ws[l].transpose(-1, -2), mask=acts[l] > 0)
            worst = max(worst, _worst(ratio, dys[l - 1], ref, tol))
        n0, k0 = ws[0].shape[-2:]
        a = above[0].reshape(G, M, n0).permute(1, 0, 2).reshape(M, G * n0)
        w = ws[0].reshape(G, n0, k0)[:, :, lo:].permute(2, 0, 1)
        ref, tol = torch_ref.gemm_oracle(a, w.reshape(k0 - lo, G * n0))
        worst = max(worst, _worst(ratio, dx0, ref, tol))
    assert native().mlp_chain_bwd_dx_f32(dy, ws, acts, G, -1)[1] is None
    print(f"f32_chain_dx {shape} M={M} G={G} nan={nan} "
          f"err/bound={worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("S", (1, 3))
@pytest.mark.parametrize("shape,M,G", CASES)
def test_dwdb_within_float64_bound(shape, M, G, S):
    ext = native()
    ws, acts, dy = _chain(shape, M, G)
    above = [*ext.mlp_chain_bwd_dx_f32(dy, ws, acts, G, -1)[0], dy]
    arena = ext.mlp_chain_bwd_dwdb_f32(above, acts, G, S)
    sizes = [w.numel() for w in ws] + [w.numel() // w.shape[-1] for w in ws]
    assert arena.shape == (S, sum(sizes))
    chunk = (-(-M // S) + 3) // 4 * 4
    for s in range(S):
        assert s * chunk < M or not arena[s].any()
    flat = torch.empty(sum(sizes), device=DEV)
    ext.reduce_arena(arena, flat, S)
    dw_db = flat.split(sizes)
    ones, worst = torch.ones(1, M, device=DEV), 0.0
    for l, w in enumerate(ws):
        n, k = w.shape[-2:]
        dyT = above[l].reshape(G, M, n).transpose(-1, -2)
        aT = acts[l].reshape(-1, M, k).transpose(-1, -2)   # x may be shared
        for out, rhs in ((dw_db[l].view(G, n, k), aT),
                         (dw_db[len(ws) + l].view(G, n, 1), ones)):
            ref, tol = torch_ref.gemm_oracle(dyT, rhs, n=M + S)
            worst = max(worst, _worst(torch_ref.gemm_bound_ratio, out, ref,
                                      tol))
    print(f"f32_chain_dwdb {shape} M={M} G={G} S={S} err/bound={worst:.4f}")
    assert worst <= 1.0


def _count(monkeypatch, name):
    ext, calls = native(), []
    real = getattr(ext, name)
    monkeypatch.setattr(ext, name, lambda *a: calls.append(1) or real(*a))
    return calls


def _public(kind, r0, split, net, x_grad=(True, True)):
    """[y, *grads] of the public forward on ``net``."""
    x1, x2, ws, bs, dy = net
    if not split:
        x1, x2 = torch.cat([x1, x2], dim=-1), None
    xs = [t.requires_grad_() for t, need in zip((x1, x2), x_grad)
          if t is not None and need and r0 == 0]
    if kind == "twin":
        y = torch.stack(Fops.twin_mlp_forward(x1, ws, bs, x2=x2))
    else:
        y = Fops.mlp_forward(x1, ws, bs, grad_row_start=r0, x2=x2)
        dy[:r0] = 0
    return [y, *torch.autograd.grad(y, [*xs, *ws, *bs], dy)]


@pytest.mark.parametrize("kind,r0,split,x_grad", [
    ("mlp", 0, False, (True, True)), ("mlp", 16, False, (True, True)),
    ("mlp", 0, True, (True, True)), ("twin", 0, True, (True, True)),
    ("twin", 0, True, (False, True))])        # dx0_lo = c1
def test_wiring_bit_for_bit(kind, r0, split, x_grad, monkeypatch):
    monkeypatch.setenv("DSAC_F32_CHAIN", "1")
    calls, res = _count(monkeypatch, "mlp_chain_bwd_dx_f32"), []
    for on in (True, False):
        if on:
            monkeypatch.setenv("DSAC_F32_CHAIN_BWD", "1")
        else:
            monkeypatch.delenv("DSAC_F32_CHAIN_BWD")
        res.append(_public(kind, r0, split,
                           _int_net(2 if kind == "twin" else 1), x_grad))
        assert len(calls) == 1      # the chain path ran, and only when on
    assert len(res[0]) == len(res[1]) == 7 + (r0 == 0) * (
        1 + split - (not x_grad[0]))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_same_bits_twice(monkeypatch):
    monkeypatch.setenv("DSAC_F32_CHAIN_BWD", "1")
    calls = _count(monkeypatch, "mlp_chain_bwd_dwdb_f32")
    x1, x2, ws, bs = _net("critic", 33, 2)
    net = (x1, x2, [w.requires_grad_() for w in ws],
           [b.requires_grad_() for b in bs], _chain("critic", 33, 2)[2])
    r1, r2 = (_public("twin", 0, True, net) for _ in range(2))
    assert len(calls) == 2
    for a, b in zip(r1, r2):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_captured_update_equals_eager(monkeypatch):
    from distributed_sac_amd.algo import SACEngine
    from tests.test_engine import small_cfg
    from tests.test_grad_clip import _gpu_replay
    monkeypatch.setenv("DSAC_F32_CHAIN", "1")
    monkeypatch.setenv("DSAC_F32_CHAIN_BWD", "1")
    dx_calls = _count(monkeypatch, "mlp_chain_bwd_dx_f32")
    dw_calls = _count(monkeypatch, "mlp_chain_bwd_dwdb_f32")
    engines = []
    for captured in (False, True):
        torch.manual_seed(0)
        cfg = small_cfg("mtsac")
        e = SACEngine(cfg, DEV, precision="fp32")
        replay = _gpu_replay(cfg)
        if captured:     # one eager warm-up update, then two replays
            e.capture(replay, cfg.batch_size, warmup_iters=1)
            e.graphed_update()
            e.graphed_update()
        else:
            for _ in range(3):
                e.update_tensors(replay.sample(cfg.batch_size,
                                               graph_safe=True))
        torch.cuda.synchronize()
        engines.append(e)
    # per update (SACEngine.update_tensors): the critic twin's backward has
    # weights that need a gradient and inputs that do not (dx walk + dW);
    # the frozen twin's has detached weights and needs only the action
    # columns (dx walk with dx0_lo = c1, no dW); the actor chain's has
    # weights that need one and a replay-sampled input (dx walk + dW)
    assert len(dx_calls) == 3 * (3 + 2) and len(dw_calls) == 2 * (3 + 2)
    for grp in ("actor_group", "critic_group", "target_group",
                "alpha_group"):
        a, b = (getattr(e, grp).flat_data for e in engines)
        assert torch.equal(a, b), grp


def test_refusals():
    ext = native()
    dy = torch.ones(5, 4, device=DEV)

    def chain(*widths):          # (ws, acts) of a chain on 5 rows
        ws = [torch.ones(n, k, device=DEV) for k, n in zip(widths, widths[1:])]
        return ws, [torch.ones(5, k, device=DEV) for k in widths[:-1]]
    ws, acts = chain(20, CAP + 1, 4)
    with pytest.raises(RuntimeError, match="width"):
        ext.mlp_chain_bwd_dx_f32(dy, ws, acts, 1, 0)
    with pytest.raises(RuntimeError, match="width"):
        ext.mlp_chain_bwd_dwdb_f32([torch.ones(5, CAP + 1, device=DEV), dy],
                                   acts, 1, 1)
    ws, acts = chain(20, 8, 4)
    bad = [acts[0], torch.ones(5, 9, device=DEV)]
    with pytest.raises(RuntimeError, match="expected"):
        ext.mlp_chain_bwd_dx_f32(dy, ws, bad, 1, 0)
    with pytest.raises(RuntimeError, match="expected"):
        ext.mlp_chain_bwd_dwdb_f32([torch.ones(5, 8, device=DEV), dy], bad,
                                   1, 1)
    with pytest.raises(RuntimeError, match="dx0_lo"):
        ext.mlp_chain_bwd_dx_f32(dy, ws, acts, 1, 21)
