"""k_f32_chain_fwd: the whole fp32 MLP forward chain in one launch
(DSAC_F32_CHAIN=1), against a float64 bound and against the per-layer path.

Observed worst err / bound of test_layers_within_float64_bound on an
MI355X, per width list: see profiles/f32_chain.md."""

import pytest
import torch

from distributed_sac_amd.ops import functional as Fops
from distributed_sac_amd.ops import native, torch_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 768          # asserted against the extension's own constant below

# (C1, C2, widths after the input)
SHAPES = {
    "critic": (53, 4, [400, 400, 400, 1]),    # odd C1, 25 tiles, N=1 head
    "unaligned": (49, 0, [400, 8]),           # K % 4 != 0, N=8
    "narrow": (64, 0, [400, 24, 400, 8]),     # stale columns, ping-pong
    "cap_in": (CAP, 0, [16]),
    "cap_mid": (20, 0, [CAP, 4]),
    "one": (4, 0, [1]),                       # L=1, one k-step
}


def _net(shape, M, G, seed=0):
    c1, c2, widths = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn(M, c1, generator=g).to(DEV)
    x2 = torch.randn(M, c2, generator=g).to(DEV) if c2 else None
    ws, bs, k = [], [], c1 + c2
    for n in widths:
        lead = (G,) if G > 1 else ()
        ws.append((torch.randn(*lead, n, k, generator=g) / k ** 0.5).to(DEV))
        bs.append(torch.randn(*lead, n, generator=g).to(DEV))
        k = n
    return x1, x2, ws, bs


CASES = [(s, M, G, False) for s in SHAPES for M in (1, 17, 33)
         for G in (1, 2)] + [("critic", 17, 2, True)]


@pytest.mark.parametrize("shape,M,G,nan", CASES)
def test_layers_within_float64_bound(shape, M, G, nan):
    ext = native()
    assert ext.F32_CHAIN_MAX_WIDTH == CAP
    x1, x2, ws, bs = _net(shape, M, G)
    if nan:
        x1[M // 2, 7] = float("nan")
    y, acts = ext.mlp_chain_fwd_f32(x1, x2, ws, bs, G, True)
    x = x1 if x2 is None else torch.cat([x1, x2], dim=-1)
    assert len(acts) == len(ws)
    assert torch.equal(acts[0].view(torch.int32), x.view(torch.int32))
    ratio = torch_ref.bound_ratio if nan else torch_ref.gemm_bound_ratio
    worst = 0.0
    for l, out in enumerate([*acts[1:], y]):
        ref, tol = torch_ref.gemm_oracle(acts[l], ws[l], bs[l],
                                         relu=l < len(ws) - 1)
        assert out.shape == ref.shape
        worst = max(worst, float(ratio(out, ref, tol).max()))
    print(f"f32_chain {shape} M={M} G={G} nan={nan} err/bound={worst:.4f}")
    assert worst <= 1.0
    if nan:
        assert torch.isnan(y[..., M // 2, :]).all()
        assert not torch.isnan(y[..., M // 2 + 1:, :]).any()


def test_save_acts_off_same_bits():
    ext = native()
    x1, x2, ws, bs = _net("critic", 33, 2)
    y, _ = ext.mlp_chain_fwd_f32(x1, x2, ws, bs, 2, True)
    y0, none = ext.mlp_chain_fwd_f32(x1, x2, ws, bs, 2, False)
    assert none == [] and torch.equal(y.view(torch.int32),
                                      y0.view(torch.int32))


def _int_net(G, dtype=torch.float32, dev=DEV):
    """53+4 -> 48 -> 20 -> 8 on small integers: every intermediate of
    forward and backward is an integer below 2^24, so any summation order
    is exact."""
    g = torch.Generator().manual_seed(3)
    M, lead = 33, ((G,) if G > 1 else ())

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).to(dev, dtype)
    x1, x2 = ints(-2, 2, M, 53), ints(-2, 2, M, 4)
    ws, bs, k = [], [], 57
    for n in (48, 20, 8):
        ws.append(ints(-1, 1, *lead, n, k).requires_grad_())
        bs.append(ints(-2, 2, *lead, n).requires_grad_())
        k = n
    return x1, x2, ws, bs, ints(-2, 2, *lead, M, 8)


def test_integer_net_is_exact_on_cpu():
    outs = []
    for dt in (torch.float32, torch.float64):
        x1, x2, ws, bs, dy = _int_net(1, dt, "cpu")
        x = torch.cat([x1, x2], dim=-1).requires_grad_()
        y = torch_ref.mlp_forward(x, ws, bs)
        outs.append([y.detach(), *torch.autograd.grad(y, [x, *ws, *bs], dy)])
    for a, b in zip(*outs):
        assert torch.equal(a.double(), b) and float(b.abs().max()) < 2 ** 24


@pytest.mark.parametrize("kind,r0,split", [("mlp", 0, False),
                                           ("mlp", 16, False),
                                           ("mlp", 0, True),
                                           ("twin", 0, True)])
def test_wiring_bit_for_bit(kind, r0, split, monkeypatch):
    G = 2 if kind == "twin" else 1
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("DSAC_F32_CHAIN", flag)
        x1, x2, ws, bs, dy = _int_net(G)
        if not split:
            x1, x2 = torch.cat([x1, x2], dim=-1), None
        xs = [t.requires_grad_() for t in (x1, x2)
              if t is not None and r0 == 0]
        if kind == "twin":
            q1, q2 = Fops.twin_mlp_forward(x1, ws, bs, x2=x2)
            y = torch.stack([q1, q2])
        else:
            y = Fops.mlp_forward(x1, ws, bs, grad_row_start=r0, x2=x2)
            dy[:r0] = 0
        res[flag] = [y, *torch.autograd.grad(y, [*xs, *ws, *bs], dy)]
    assert len(res["1"]) == len(res["0"]) == 7 + (r0 == 0) * (1 + split)
    for a, b in zip(res["1"], res["0"]):
        assert torch.equal(a, b)


def test_captured_update_equals_eager(monkeypatch):
    from distributed_sac_amd.algo import SACEngine
    from tests.test_engine import small_cfg
    from tests.test_grad_clip import _gpu_replay
    monkeypatch.setenv("DSAC_F32_CHAIN", "1")
    ext, calls = native(), []
    real = ext.mlp_chain_fwd_f32
    monkeypatch.setattr(ext, "mlp_chain_fwd_f32",
                        lambda *a: calls.append(1) or real(*a))
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
    # per update: actor chain, target twin, critic twin, frozen twin
    assert len(calls) == 4 * (3 + 2)
    for grp in ("actor_group", "critic_group", "target_group",
                "alpha_group"):
        a, b = (getattr(e, grp).flat_data for e in engines)
        assert torch.equal(a, b), grp


def test_refusals_and_fallback(monkeypatch):
    ext = native()
    x = torch.ones(5, 20, device=DEV)

    def wb(n, k):
        return torch.ones(n, k, device=DEV), torch.ones(n, device=DEV)
    w0, b0 = wb(CAP + 1, 20)
    w1, b1 = wb(4, CAP + 1)
    with pytest.raises(RuntimeError, match="width"):
        ext.mlp_chain_fwd_f32(x, None, [w0, w1], [b0, b1], 1, True)
    with pytest.raises(RuntimeError, match="expected"):
        ext.mlp_chain_fwd_f32(x, None, [wb(8, 20)[0], wb(4, 9)[0]],
                              [wb(8, 20)[1], b1], 1, True)
    ys = []
    for flag in ("1", "0"):
        monkeypatch.setenv("DSAC_F32_CHAIN", flag)
        ys.append(Fops.mlp_forward(x, [w0, w1], [b0, b1]))
    assert torch.equal(ys[0], ys[1])
