"""The squash kernels (k_squash_fwd, k_squash_bwd, k_squash_bwd2) and the
attention-pool kernels (k_attn_pool_fwd, k_attn_pool_bwd) against the
float64 oracles of ops/torch_ref.py.  Every element of every output is
compared with its own bound (docs/KERNELS.md "Numerics"); the inputs, the
``*_ratios`` helpers and the proof that the bounds hold for a correct
kernel and break for a faulty one are in tests/test_squash_oracle.py.

logp, act and both backwards are judged from the kernel's own saved
tanh / log-std / eps (teacher forcing), tanh itself from the inputs, and
the counter-mode eps from the hash.  The worst err / bound per output is
printed (collected in profiles/squash_reference.md).
"""

import pytest
import torch

from tests.test_squash_oracle import (
    BF, COUNTERS, KRNG_SHAPES, POOL_D, POOL_E, POOL_HC, POOL_LOGITS, POOL_M,
    SQ_A, SQ_B, SQ_K, SQ_LAYOUTS, assert_inside, bwd_ratios, eps_ratio,
    fwd_ratios, pool_bwd_inputs, pool_bwd_ratios, pool_fwd_ratios,
    pool_inputs, squash_inputs, squash_layout)

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ext():
    from distributed_sac_amd.ops import native
    return native()


def _fwd(ext, mu_v, lsr_v, eps, k, ctr=None):
    act, logp, t, ls = ext.squashed_gaussian_fwd(mu_v, lsr_v, eps, k, ctr)
    return dict(act=act.cpu(), logp=logp.cpu(), t=t.cpu(), ls=ls.cpu())


@pytest.mark.parametrize("A", SQ_A)
@pytest.mark.parametrize("B", SQ_B)
def test_squash_fwd_bwd(B, A):
    """Given eps: forward in three layouts, then k_squash_bwd and
    k_squash_bwd2 on the forward's own outputs with a single and a twin
    action gradient and a contiguous and a strided raw log-std."""
    ext = _ext()
    inp = squash_inputs(B, A)
    d = {n: inp[n].to(DEV) for n in ("mu", "lsr", "eps", "ga", "gl")}
    for k in SQ_K:
        for layout in SQ_LAYOUTS:
            mu_v, lsr_v = squash_layout(d["mu"], d["lsr"], layout)
            out = _fwd(ext, mu_v, lsr_v, d["eps"], k)
            assert_inside(fwd_ratios(inp["mu"], inp["lsr"], inp["eps"], k,
                                     out), f"fwd {B}x{A} k={k} {layout}")
            # a NaN in mu or in the raw log-std: that row's logp, no other
            nan = torch.isnan(out["logp"]).reshape(-1).nonzero().reshape(-1)
            assert nan.tolist() == inp["nan_rows"]
        if inp["nan_rows"]:
            assert bool(torch.isnan(out["ls"][2, A - 1]))
            assert bool(torch.isnan(out["t"][2, A - 1]))
        ls, t = out["ls"].to(DEV), out["t"].to(DEV)
        for ga, ga_d in ((inp["ga"][0], d["ga"][0].contiguous()),
                         (inp["ga"], d["ga"])):
            args = (ga, inp["gl"], inp["lsr"], out["ls"], inp["eps"],
                    out["t"], k)
            tag = f"{B}x{A} k={k} ga{tuple(ga.shape)}"
            if ga.dim() == 2:
                du, dlsr = ext.squashed_gaussian_bwd(
                    ga_d, d["gl"], d["lsr"], ls, d["eps"], t, k)
                assert_inside(bwd_ratios(*args, du=du.cpu(),
                                         dlsr=dlsr.cpu()), "bwd " + tag)
            for layout in ("contig", "head_rows"):
                lsr_v = squash_layout(d["mu"], d["lsr"], layout)[1]
                dhead = ext.squashed_gaussian_bwd2(
                    ga_d, d["gl"], lsr_v, ls, d["eps"], t, k).cpu()
                assert dhead.dtype == BF
                assert_inside(bwd_ratios(*args, dhead=dhead),
                              f"bwd2 {tag} {layout}")
                if inp["nan_rows"]:
                    # the NaN log-std reaches its own gradient element
                    assert bool(torch.isnan(dhead[2, 2 * A - 1]))
                    assert bool(torch.isnan(dhead[1, 0]))


def test_squash_bwd_nan_action_gradient():
    """A NaN in either head of the action gradient reaches dhead."""
    ext = _ext()
    B, A, k = 257, 4, 2.5
    inp = squash_inputs(B, A)
    inp["ga"][1, 5, 2] = float("nan")
    d = {n: inp[n].to(DEV) for n in ("mu", "lsr", "eps", "ga", "gl")}
    out = _fwd(ext, d["mu"], d["lsr"], d["eps"], k)
    ls, t = out["ls"].to(DEV), out["t"].to(DEV)
    dhead = ext.squashed_gaussian_bwd2(d["ga"], d["gl"], d["lsr"], ls,
                                       d["eps"], t, k).cpu()
    assert bool(torch.isnan(dhead[5, 2])) and bool(torch.isnan(dhead[5, A + 2]))
    assert_inside(bwd_ratios(inp["ga"], inp["gl"], inp["lsr"], out["ls"],
                             inp["eps"], out["t"], k, dhead=dhead),
                  "bwd2 NaN ga")
    du, dlsr = ext.squashed_gaussian_bwd(
        d["ga"][1].contiguous(), d["gl"], d["lsr"], ls, d["eps"], t, k)
    assert bool(torch.isnan(du[5, 2])) and bool(torch.isnan(dlsr[5, 2]))


@pytest.mark.parametrize("ctr", COUNTERS)
@pytest.mark.parametrize("B,A", KRNG_SHAPES)
def test_squash_counter_mode(B, A, ctr):
    """The in-kernel Box-Muller draw equals the hashed float64 draw element
    for element; the other outputs follow from that saved eps; the same
    counter gives the same bits."""
    ext = _ext()
    inp = squash_inputs(B, A)
    mu, lsr = inp["mu"].to(DEV), inp["lsr"].to(DEV)
    c = torch.tensor([ctr], dtype=torch.int64, device=DEV)
    k = 2.5
    eps = torch.full((B, A), float("nan"), device=DEV)
    mu_v, lsr_v = squash_layout(mu, lsr, "head")
    out = _fwd(ext, mu_v, lsr_v, eps, k, c)
    e = eps.cpu()
    assert_inside(eps_ratio(e, ctr), f"eps {B}x{A} c={ctr}")
    assert_inside(fwd_ratios(inp["mu"], inp["lsr"], e, k, out),
                  f"fwd krng {B}x{A} c={ctr}")
    eps2 = torch.empty(B, A, device=DEV)
    _fwd(ext, mu, lsr, eps2, k, c)
    assert torch.equal(e, eps2.cpu())


def _pool_cases(E, D):
    for Mz in POOL_M:
        for kind in POOL_LOGITS:
            yield Mz, kind


@pytest.mark.parametrize("D", POOL_D)
@pytest.mark.parametrize("E", POOL_E)
def test_attn_pool_fwd(E, D):
    """Legacy mode, and enc mode with rep 1 and 2 at three hc widths
    (70 + D spans more than one pass of the 64 lanes)."""
    ext = _ext()
    for Mz, kind in _pool_cases(E, D):
        logits, z, _ = pool_inputs(Mz, E, D, 1, kind)
        alpha, pooled = ext.attn_pool_fwd(logits.to(DEV), z.to(DEV))
        assert pooled.dtype == BF and tuple(pooled.shape) == (Mz, D)
        assert_inside(pool_fwd_ratios(logits, z, 1, alpha.cpu(),
                                      pooled.cpu()),
                      f"pool fwd {Mz}x{E}x{D} {kind}")
        for rep in (1, 2):
            for zc in POOL_HC:
                logits, z, hc = pool_inputs(Mz, E, D, rep, kind, zc)
                alpha, enc = ext.attn_pool_fwd_enc(
                    logits.to(DEV), z.to(DEV), hc.to(DEV), rep)
                assert tuple(alpha.shape) == (Mz, E)
                assert tuple(enc.shape) == (Mz * rep, zc + D)
                enc = enc.cpu()
                assert_inside(
                    pool_fwd_ratios(logits, z, rep, alpha.cpu(),
                                    enc[:, zc:], hc, enc[:, :zc]),
                    f"pool enc {Mz}x{E}x{D} rep={rep} zc={zc} {kind}")


@pytest.mark.parametrize("D", POOL_D)
@pytest.mark.parametrize("E", POOL_E)
def test_attn_pool_bwd(E, D):
    ext = _ext()
    for Mz, kind in _pool_cases(E, D):
        for ld, off in ((D, 0), (D + 9, 4)):
            z, alpha, dz_full = pool_bwd_inputs(Mz, E, D, ld, kind)
            dzencs, dl = ext.attn_pool_bwd(z.to(DEV), alpha.to(DEV),
                                           dz_full.to(DEV), ld, off)
            assert_inside(
                pool_bwd_ratios(z, alpha, dz_full[:, off:off + D],
                                dzencs.cpu(), dl.cpu()),
                f"pool bwd {Mz}x{E}x{D} ld={ld} off={off} {kind}")
