"""The LayerNorm chain kernels against float64, layer by layer on the
kernel's own saved tensors (the method of test_gemm_reference.py): forward
h / xhat / rstd from the bf16 output of the layer before, backward dz from the
kernel's own dz of the layer above, the d gamma / d beta fold against float64
column sums.  Bounds: torch_ref.ln_fwd_oracle / ln_bwd_oracle / ln_colsum
(derived from the arithmetic, profiles/layer_norm.md)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from distributed_sac_amd.ops import torch_ref as R  # noqa: E402

DEV = "cuda"

# name: M, widths, G, columns of x1 (the rest is x2; 0 = one input), special
CASES = {
    # odd K0, a 40-wide layer whose last tile is half pad columns, a partial
    # row tile, twin groups, an N = 1 head, input x1 || x2
    "pad_cols_twin": (37, [53, 40, 72, 1], 2, 39, None),
    # CMAX: two column passes per wave; 400: three waves own no tile
    "cmax_idle_waves": (19, [768, 768, 400, 8], 1, 0, None),
    # one tile, N = 16: the smallest LN
    "one_tile": (16, [32, 16, 1], 2, 0, None),
    # zero weights and one bias value in layer 1: z constant, var = 0
    "zero_variance": (20, [24, 32, 16, 1], 1, 0, "const"),
    # |mu| >> sigma: E[z^2] - mu^2 in fp32 has no correct digit left
    "bias_1000": (20, [24, 32, 16, 1], 2, 0, "bias"),
}


def _ok(out, ref, tol):
    r = R.gemm_bound_ratio(out, ref, tol)
    print("  worst err/bound", float(r.max()))
    return bool(torch.isfinite(r).all())


@pytest.mark.parametrize("name", list(CASES))
def test_ln_chain(name):
    from distributed_sac_amd import ops
    from distributed_sac_amd.ops.chain import ManualChain, pack_chains
    from distributed_sac_amd.ops.flat import FlatParams
    ext = ops.native()
    M, widths, G, c1, special = CASES[name]
    gen = torch.Generator().manual_seed(5)
    L = len(widths) - 1

    def P(*shape, scale=1.0, shift=0.0):
        return torch.nn.Parameter(
            (torch.randn(*shape, generator=gen) * scale + shift).to(DEV))
    ws = [P(G, N, K, scale=K ** -0.5)
          for K, N in zip(widths[:-1], widths[1:])]
    bs = [P(G, N, scale=0.3) for N in widths[1:]]
    gam = [P(G, N, scale=0.4, shift=1.0) for N in widths[1:-1]]
    bet = [P(G, N, scale=0.3) for N in widths[1:-1]]
    with torch.no_grad():
        if special == "const":
            ws[1].zero_()
            bs[1].fill_(0.25)
        if special == "bias":
            bs[0].add_(1000.0)
    group = FlatParams(ws + bs + gam + bet)
    w16 = [w.detach().to(torch.bfloat16) for w in ws]
    det = lambda ps: [p.detach() for p in ps]   # noqa: E731
    ch = ManualChain(w16, det(bs), G=G, group=group, w_params=ws,
                     b_params=bs, gammas=det(gam), betas=det(bet),
                     g_params=gam, be_params=bet)
    pack_chains(ext, [(ch, True, True)])
    x = torch.randn(M, widths[0], generator=gen).to(DEV)
    if special == "const":
        x[:] = x[0]
    y, acts = ch.forward(x[:, :c1], x[:, c1:]) if c1 else ch.forward(x)
    hs, xhs, rs = (acts[1 + i * (L - 1):1 + (i + 1) * (L - 1)]
                   for i in range(3))
    assert torch.equal(acts[0], x.to(torch.bfloat16))
    y0 = ch.forward(x, save_acts=False)[0]      # the no-grad forward
    assert torch.equal(y0, y)

    # ---- forward, layer by layer -------------------------------------
    a = acts[0].expand(G, M, -1)
    for li in range(L - 1):
        (h, xh, r), (th, tx, tr) = R.ln_fwd_oracle(
            a, w16[li], bs[li].detach(), gam[li].detach(), bet[li].detach())
        print(name, "layer", li)
        assert _ok(hs[li].view(G, M, -1), h, th)
        assert _ok(xhs[li].view(G, M, -1), xh, tx)
        assert _ok(rs[li], r, tr)
        a = hs[li].view(G, M, -1)
    assert _ok(y.view(G, M, -1), *R.gemm_oracle(a, w16[-1], bs[-1].detach()))

    # ---- backward ------------------------------------------------------
    dy = torch.randn(G, M, widths[-1], generator=gen).to(DEV) \
        .to(torch.bfloat16)
    dy = dy if G > 1 else dy[0]
    lo_in = widths[0] // 2 + 1
    outs = ch._ln_dx(ext, dy, acts, 1, lo_in)
    dzs, parts = outs[:L], outs[L:2 * L - 1]
    terms = []
    for li in range(L - 2, -1, -1):
        dz, db, dg = R.ln_bwd_oracle(
            dzs[li + 1], w16[li + 1], hs[li].view(G, M, -1),
            xhs[li].view(G, M, -1), rs[li], gam[li].detach())
        print(name, "backward layer", li)
        assert _ok(dzs[li], *dz)
        terms.insert(0, (db, dg))
    for lo in (-1, 0, lo_in):
        nodw = ch._ln_dx(ext, dy, acts, 0, lo)
        if lo < 0:
            assert len(nodw) == 0
            continue
        dx0 = outs[-1] if lo == lo_in else ch._ln_dx(ext, dy, acts, 1, lo)[-1]
        assert torch.equal(nodw[-1], dx0)       # want_dw = 0: the same bits
        assert _ok(dx0, *R.gemm_oracle(
            dzs[0], w16[0].transpose(-1, -2)[:, lo:, :].contiguous()))

    # ---- the d gamma / d beta fold --------------------------------------
    for chunk in (16, 64):
        S = -(-M // chunk)
        arenas = []
        for _ in range(2):
            arena = torch.full((S, group.numel), float("nan"), device=DEV)
            ext.ln_dgb_fold(list(parts), arena, ch.g_offs, ch.be_offs, G, S,
                            chunk, M)
            arenas.append(arena)
        assert torch.equal(arenas[0].nan_to_num(7.0),
                           arenas[1].nan_to_num(7.0))      # fixed order
        for li, (db, dg) in enumerate(terms):
            N = widths[li + 1]
            for off, term in ((ch.be_offs[li], db), (ch.g_offs[li], dg)):
                for s in range(S):
                    got = arenas[0][s, off:off + G * N].view(G, N)
                    ref, tol = R.ln_colsum(*term, s * chunk,
                                           min(M, (s + 1) * chunk))
                    assert _ok(got, ref, tol), (chunk, li, s)
