"""The five public MLP entry points of ops/functional.py (mlp_forward,
twin_mlp_forward, mlp_forward_bf16, twin_mlp_forward_bf16,
grouped_mlp_bf16), forward and every gradient: what the argument layout of
the two autograd Functions, the x1 / x2 column split and the
needs_input_grad arithmetic are trusted for.

fp32 is compared with plain torch.nn.functional.linear autograd at the
tolerances of tests/test_gpu_kernels.py (test_twin_mlp_autograd).  bf16 is
held to the float64 bounds of tests/test_gemm_reference.py: every layer is
judged from its own bf16 operands, which the per-layer bindings (checked
there) reproduce bit for bit.

Shapes: batch 1, 5 and 70 (70 crosses the 64-row tile), input width 7
(whole, or x1 4 columns + x2 3 columns), hidden widths 33 and 64, output
width 1 and 6, 1 and 3 layers.
"""

import functools

import pytest
import torch

from distributed_sac_amd.ops import functional as Fops
from distributed_sac_amd.ops import native
from distributed_sac_amd.ops import torch_ref as R
from tests.test_gemm_reference import _check, _dwdb_splits

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
K0, C1 = 7, 4                       # input width; x1's share of it
HIDDEN = {1: [], 3: [33, 64]}       # layers -> hidden widths
GRID = [(M, L, out) for M in (1, 5, 70) for L in (1, 3) for out in (1, 6)]


def _net(G, M, L, out, r0):
    """x, ws [G,N,K], bs [G,N], dy [G,M,out] (no G dimension when G == 1);
    dy is zero in the rows below r0."""
    gen = torch.Generator().manual_seed(1000 * M + 100 * L + 10 * out + G)
    lead = (G,) if G > 1 else ()

    def rn(*shape):
        return torch.randn(*shape, generator=gen).to(DEV)
    x, ws, bs, k = rn(M, K0), [], [], K0
    for n in [*HIDDEN[L], out]:
        ws.append(rn(*lead, n, k) / k ** 0.5)
        bs.append(rn(*lead, n))
        k = n
    dy = rn(*lead, M, out)
    dy[..., :r0, :] = 0
    return x, ws, bs, dy


def _count(monkeypatch, name):
    ext, calls = native(), []
    real = getattr(ext, name)
    monkeypatch.setattr(ext, name, lambda *a: calls.append(1) or real(*a))
    return calls


# ---------------------------------------------------------------------------
# fp32: mlp_forward (G = 1), twin_mlp_forward (G = 2)
# ---------------------------------------------------------------------------

@pytest.fixture(params=[(f, b) for f in "01" for b in "01"],
                ids=lambda p: f"chain{p[0]}-bwd{p[1]}")
def chain_flags(request, monkeypatch):
    monkeypatch.setenv("DSAC_F32_CHAIN", request.param[0])
    monkeypatch.setenv("DSAC_F32_CHAIN_BWD", request.param[1])


@functools.lru_cache(maxsize=None)
def _f32_ref(G, M, L, out, r0):
    """The net and (y, dx, dws, dbs) of torch's own linear autograd."""
    x, ws, bs, dy = _net(G, M, L, out, r0)
    xr = x.clone().requires_grad_()
    wr = [w.clone().requires_grad_() for w in ws]
    br = [b.clone().requires_grad_() for b in bs]
    heads = []
    for g in range(G):
        h = xr
        for i in range(L):
            w, b = (wr[i][g], br[i][g]) if G > 1 else (wr[i], br[i])
            h = torch.nn.functional.linear(h, w, b)
            if i < L - 1:
                h = torch.relu(h)
        heads.append(h)
    y = torch.stack(heads) if G > 1 else heads[0]
    grads = torch.autograd.grad(y, [xr, *wr, *br], dy)
    return (x, ws, bs, dy), (y.detach(), grads[0], grads[1:1 + L],
                             grads[1 + L:])


# G, M, L, out, grad_row_start, x given as x1 + x2, which of them need a
# gradient, layer 0 frozen
F32_CASES = (
    [(G, M, L, out, 0, False, (True,), False)
     for G in (1, 2) for M, L, out in GRID]
    # x1 only, x2 only (the dx0_lo = c1 shortcut of the chain backward; a
    # single layer stays per-layer and splits a full-width dx), both
    + [(G, 70, L, 6, 0, True, need, False) for G in (1, 2) for L in (1, 3)
       for need in ((True, False), (False, True), (True, True))]
    + [(1, 5, 3, 6, 3, split, (False, False), False)
       for split in (False, True)]
    + [(G, 5, 3, 6, 0, True, (False, True), True) for G in (1, 2)])


@pytest.mark.parametrize("G,M,L,out,r0,split,need_x,frozen", F32_CASES)
def test_f32_entry_points(G, M, L, out, r0, split, need_x, frozen,
                          chain_flags):
    """``frozen``: layer 0's weight and bias do not require a gradient (dW
    and db come from one launch, keyed on the weight, as the engines'
    detached twin has them): they get none, every other gradient is the
    reference's."""
    (x, ws, bs, dy), (y_ref, dx_ref, dws_ref, dbs_ref) = _f32_ref(
        G, M, L, out, r0)
    if split:
        xs = [x[:, :C1].clone(), x[:, C1:].clone()]
        dxs_ref = [dx_ref[:, :C1], dx_ref[:, C1:]]
    else:
        xs, dxs_ref = [x.clone()], [dx_ref]
    for t, need in zip(xs, need_x):
        t.requires_grad_(need)
    wl = [w.clone().requires_grad_(not (frozen and i == 0))
          for i, w in enumerate(ws)]
    bl = [b.clone().requires_grad_(not (frozen and i == 0))
          for i, b in enumerate(bs)]
    x2 = xs[1] if split else None
    if G == 1:
        y = Fops.mlp_forward(xs[0], wl, bl, grad_row_start=r0, x2=x2)
    else:
        y = torch.stack(Fops.twin_mlp_forward(xs[0], wl, bl, x2=x2))
    assert y.shape == y_ref.shape
    assert torch.allclose(y, y_ref, atol=1e-4, rtol=1e-4)
    y.backward(dy)
    named = ([(f"dx{i + 1}", t, r) for i, (t, r) in
              enumerate(zip(xs, dxs_ref))]
             + [(f"dw{i}", t, r) for i, (t, r) in enumerate(zip(wl, dws_ref))]
             + [(f"db{i}", t, r) for i, (t, r) in enumerate(zip(bl, dbs_ref))])
    for name, t, ref in named:
        if not t.requires_grad:
            assert t.grad is None, name
            continue
        assert t.grad is not None and t.grad.shape == ref.shape, name
        err = float((t.grad - ref).abs().max())
        print(f"f32 {name} max err {err:.3e}")
        assert torch.allclose(t.grad, ref, atol=1e-4, rtol=1e-3), name


# ---------------------------------------------------------------------------
# bf16: mlp_forward_bf16 (G = 1), twin_mlp_forward_bf16 (G = 2),
# grouped_mlp_bf16 (G = 3, transposed parameters)
# ---------------------------------------------------------------------------

def _g3(t, G):
    """[G, rows, cols] of a tensor the bindings give without a group
    dimension when G == 1."""
    return t.reshape(G, *t.shape[-2:])


# G, M, L, out, grad_row_start, x needs a gradient, layer 0 frozen
BF16_CASES = (
    [(G, M, L, out, 0, True, False) for G in (1, 2, 3) for M, L, out in GRID]
    + [(1, 5, 3, 6, 3, False, False)]
    + [(G, 5, 3, 6, 0, False, False) for G in (1, 2, 3)]
    + [(G, 5, 3, 6, 0, True, True) for G in (1, 2, 3)])


@pytest.mark.parametrize("G,M,L,out,r0,need_x,frozen", BF16_CASES)
def test_bf16_entry_points(G, M, L, out, r0, need_x, frozen, monkeypatch):
    """The output and every gradient inside the float64 bound of the GEMM
    that produced it; dW/db launched for exactly the layers whose weight
    requires a gradient, dx when x does."""
    ext = native()
    x, ws, bs, dy = _net(G, M, L, out, r0)
    w16 = [w.to(BF) for w in ws]
    x = x.requires_grad_(need_x)
    transposed = G == 3
    if transposed:     # the mixture's parameters: W (k,in,out), b (k,1,out)
        ws = [w.transpose(1, 2).contiguous() for w in ws]
        bs = [b.unsqueeze(1).contiguous() for b in bs]
    for i in range(L):
        ws[i].requires_grad_(not (frozen and i == 0))
        bs[i].requires_grad_(not (frozen and i == 0))
    dwdb_calls = _count(monkeypatch, "linear_bwd_dwdb_bf16")
    if G == 1:
        y = Fops.mlp_forward_bf16(x, ws, bs, w16, grad_row_start=r0)
    elif G == 2:
        y = torch.stack(Fops.twin_mlp_forward_bf16(x, ws, bs, w16))
    else:
        y = Fops.grouped_mlp_bf16(x, ws, bs, w16, G)
    assert y.dtype == torch.float32 and y.shape == dy.shape
    y.backward(dy)
    assert len(dwdb_calls) == L - frozen

    # each layer's own bf16 operands, from the per-layer bindings
    b2 = [b.detach().reshape(G, -1) if G > 1 else b.detach() for b in bs]
    acts = [x.detach().to(BF)]
    for i in range(L - 1):
        acts.append(ext.linear_act_fwd_bf16(acts[-1], w16[i], b2[i], 1, G, 0))
    ref, tol = R.gemm_oracle(acts[-1], w16[-1], b2[-1])
    _check("entry point", "fp32 output", _g3(y.detach(), G), _g3(ref, G),
           _g3(tol, G))

    Mg = M - r0
    acts = [a[..., r0:, :] for a in acts]
    d = dy[..., r0:, :].contiguous().to(BF)
    for i in range(L - 1, -1, -1):
        act = int(i < L - 1)
        yout = acts[i + 1] if act else acts[i]
        dm = torch.where(yout != 0, d, torch.zeros_like(d)) if act else d
        N, K = w16[i].shape[-2:]
        dw, db = ws[i].grad, bs[i].grad
        if frozen and i == 0:
            assert dw is None and db is None
        else:
            if transposed:
                assert dw.shape == ws[i].shape and db.shape == bs[i].shape
                dw = dw.transpose(1, 2)
            n = Mg + _dwdb_splits(Mg, N, K, G)
            dmT = _g3(dm, G).transpose(1, 2)
            # layer 0's input is shared by the groups
            ref, tol = R.gemm_oracle(
                dmT, _g3(acts[i], 1 if i == 0 else G).transpose(1, 2), n=n)
            _check("entry point", "fp32 dW", _g3(dw, G), ref, tol)
            ref, tol = R.gemm_oracle(dmT, torch.ones(1, 1, Mg, device=DEV),
                                     n=n)
            _check("entry point", "fp32 db", db.reshape(G, N, 1), ref, tol)
        if i > 0:
            d = ext.linear_bwd_dx_bf16(d, w16[i], yout, act, G, 0)
        elif need_x:
            # one sum over the G * N terms of all groups; the kernel's bf16
            # result comes back widened to fp32
            assert r0 == 0 and x.grad.dtype == torch.float32
            ref, tol = R.gemm_oracle(
                _g3(dm, G).permute(1, 0, 2).reshape(1, M, G * N),
                _g3(w16[0], G).permute(2, 0, 1).reshape(1, K, G * N))
            _check("entry point", "bf16 dx", x.grad.to(BF).reshape(1, M, K),
                   ref, tol)
        else:
            assert x.grad is None
