"""The float64 squash / attention-pool oracles of ops/torch_ref.py, checked
without a GPU (the counterpart of tests/test_gemm_oracle.py).

(a) An fp32 torch emulation of each kernel's operation sequence —
    k_squash_fwd (both eps modes), k_squash_bwd / k_squash_bwd2,
    k_attn_pool_fwd (legacy and enc mode), k_attn_pool_bwd — stays inside
    every bound at every shape tests/test_squash_reference.py runs on the
    GPU.
(b) The same emulation with one of fourteen faults (a wrong stride, swapped
    halves, a lost factor, a wrong sign, a wrong hash input ...) leaves at
    least one bound: the check is sensitive.
(c) The transcendental allowances E_exp, E_log, E_tanh, E_cos are four
    times the worst ulp error (rounded up, at least 1) of the fp32 torch
    call against float64 over these inputs.
(d) The float64 eps oracle is standard normal and uncorrelated (the GPU
    test shows the kernel's draw equals it element for element).

This module also holds the deterministic inputs and the ``*_ratios``
helpers both test files use.
"""

import math

import pytest
import torch

from distributed_sac_amd.ops import torch_ref as R

F32 = torch.float32
BF = torch.bfloat16
INF = float("inf")

SQ_B = [1, 255, 256, 257, 513]
SQ_A = [1, 4, 32]
SQ_K = [1.0, 2.5]
SQ_LAYOUTS = ["contig", "head", "head_rows"]
SQ_B0 = 3                               # rows in front of the row-offset view
KRNG_SHAPES = [(1, 1), (257, 4), (513, 32)]
COUNTERS = [0, 42, 2 ** 31 - 3]
POOL_M = [1, 3, 4, 5, 37]
POOL_E = [1, 6, 16]
POOL_D = [1, 50, 64]
POOL_HC = [1, 12, 70]
POOL_LOGITS = ["normal", "equal", "big"]


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def squash_inputs(B, A):
    """Deterministic fp32 inputs of one shape: raw log-std exactly -20 and
    2, the next fp32 outside either, and +-50 among N(-1, 1.5) values;
    eps with exact zeros; mu such that u = mu + s eps covers [-25, 25],
    cubically dense near 0 (|u| < 4 well conditioned, 4 < |u| < 9 ill
    conditioned, beyond that t = +-1 exactly); a twin action gradient and
    a logp gradient with exact zeros; from B = 3 on, one NaN in mu (row 1)
    and one in the raw log-std (row 2)."""
    g = torch.Generator().manual_seed(1000 * B + A)
    n = B * A
    j = torch.arange(n)
    lsr = torch.randn(n, generator=g) * 1.5 - 1.0
    lo, hi = torch.tensor(-20.0), torch.tensor(2.0)
    ninf, pinf = torch.tensor(-INF), torch.tensor(INF)
    specials = [lo, hi, torch.nextafter(lo, ninf), torch.nextafter(hi, pinf),
                torch.tensor(50.0), torch.tensor(-50.0)]
    for q, v in enumerate(specials):
        lsr[(j % 13) == 2 * q + 1] = v
    eps = torch.randn(n, generator=g)
    eps[(j % 7) == 3] = 0.0
    x = torch.linspace(-1.0, 1.0, n)[torch.randperm(n, generator=g)]
    s = torch.exp(torch.clamp(lsr, -20.0, 2.0))
    mu = 25.0 * x ** 3 - s * eps
    ga = torch.randn(2, n, generator=g)
    gl = torch.randn(B, generator=g)
    gl[(torch.arange(B) % 5) == 4] = 0.0
    mu, lsr, eps = (v.reshape(B, A).contiguous() for v in (mu, lsr, eps))
    nan_rows = []
    if B >= 3:
        mu[1, 0] = float("nan")
        lsr[2, A - 1] = float("nan")
        nan_rows = [1, 2]
    return dict(mu=mu, lsr=lsr, eps=eps, ga=ga.reshape(2, B, A), gl=gl,
                nan_rows=nan_rows)


def squash_layout(mu, lsr, layout):
    """``(mu_view, lsr_view)`` on the tensors' device: contiguous, the two
    halves of a joined [B, 2A] head, or those of a head that starts
    SQ_B0 rows into a taller one."""
    if layout == "contig":
        return mu, lsr
    head = torch.cat([mu, lsr], 1)
    if layout == "head_rows":
        junk = torch.full((SQ_B0, head.shape[1]), 7.0, device=head.device)
        head = torch.cat([junk, head], 0)[SQ_B0:]
    A = mu.shape[1]
    return head[:, :A], head[:, A:]


def pool_inputs(Mz, E, D, rep, kind, zc=0):
    g = torch.Generator().manual_seed(7 + 131 * Mz + 17 * E + D + 1009 * rep)
    M = Mz * rep
    if kind == "normal":
        logits = torch.randn(Mz, E, generator=g)
    elif kind == "equal":
        logits = torch.full((Mz, E), 0.75)
    else:                       # +-1e4, a little apart: needs the max shift
        sign = (torch.arange(Mz * E).reshape(Mz, E) % 3 == 0).float() * 2 - 1
        logits = sign * 1e4 + torch.randn(Mz, E, generator=g)
    z = torch.randn(E, M, D, generator=g)
    hc = torch.randn(Mz, max(zc, 1), generator=g).to(BF)
    return logits, z, hc


def pool_bwd_inputs(M, E, D, ld, kind):
    logits, z, _ = pool_inputs(M, E, D, 1, kind)
    g = torch.Generator().manual_seed(99 + M + E + D + ld)
    alpha = torch.softmax(logits, -1)
    dz_full = torch.randn(M, ld, generator=g).to(BF).contiguous()
    return z, alpha, dz_full


# ---------------------------------------------------------------------------
# err / bound of a set of outputs (CPU tensors), shared with the GPU tests
# ---------------------------------------------------------------------------

def _same_bits(out, want):
    """0.0 if fp32 ``out`` equals ``want`` bit for bit (any NaN matching
    any NaN), else inf."""
    if out.shape != want.shape:
        return INF
    o, w = out.contiguous(), want.contiguous()
    same = (o.view(torch.int32) == w.view(torch.int32)) \
        | (torch.isnan(o) & torch.isnan(w))
    return 0.0 if bool(same.all()) else INF


def _worst(out, ref, tol):
    r = R.bound_ratio(out, ref, tol)
    return float(r.max()) if r.numel() else 0.0


def fwd_ratios(mu, lsr, eps, k, out):
    """Worst err / bound per output of one squash forward; ``out`` holds
    the CPU fp32 ``act, logp, t, ls``.  logp and act are judged from the
    output's own ``t``."""
    o = R.squash_fwd_oracle(mu, lsr, eps, k, t=out["t"])
    return {
        "ls_out": _same_bits(out["ls"], o["ls"]),
        "tanh_u": _worst(out["t"], o["t"], o["tol_t"]),
        "act": _same_bits(out["act"], o["act"]),
        "logp": _worst(out["logp"].reshape(-1, 1), o["logp"], o["tol_logp"]),
    }


def bwd_ratios(ga, gl, lsr, ls, eps, t, k, du=None, dlsr=None, dhead=None):
    """Worst err / bound of k_squash_bwd's fp32 ``du, dlsr`` or of
    k_squash_bwd2's joined bf16 ``dhead``."""
    rdu, rdl, tdu, tdl = R.squash_bwd_oracle(ga, gl, lsr, ls, eps, t, k)
    A = rdu.shape[1]
    if dhead is not None:
        if tuple(dhead.shape) != (rdu.shape[0], 2 * A):
            return {"dhead.du": INF, "dhead.dlsr": INF}
        return {"dhead.du": _worst(dhead[:, :A], rdu, tdu),
                "dhead.dlsr": _worst(dhead[:, A:], rdl, tdl)}
    return {"du": _worst(du, rdu, tdu), "dlsr": _worst(dlsr, rdl, tdl)}


def eps_ratio(e, ctr):
    """Worst err / bound of a saved counter-mode eps [B, A] (fp32)."""
    e64, r = R.squash_eps_oracle(ctr, e.shape[0], e.shape[1])
    return {"eps": _worst(e, e64, R.SQ_EPS_BOUND * (r + 1.0))}


def pool_fwd_ratios(logits, z, rep, alpha, pooled, hc=None, enc_hc=None):
    a64, ta, p64, tp = R.attn_pool_oracle(logits, z, rep)
    r = {"alpha": _worst(alpha, a64, ta), "pooled": _worst(pooled, p64, tp)}
    if logits.shape[1] == 1:
        r["alpha==1"] = 0.0 if bool((alpha == 1.0).all()) else INF
    if hc is not None:
        want = hc.repeat(rep, 1)
        r["hc"] = 0.0 if enc_hc.shape == want.shape and \
            torch.equal(enc_hc.view(torch.int16), want.view(torch.int16)) \
            else INF
    return r


def pool_bwd_ratios(z, alpha, dz, dzencs, dlogits):
    bits, d64, tol = R.attn_pool_bwd_oracle(z, alpha, dz)
    got = dzencs.contiguous().view(torch.int16).long() & 0xFFFF
    r = {"d_zencs": 0.0 if torch.equal(got, bits) else INF,
         "dlogits": _worst(dlogits, d64, tol)}
    if z.shape[0] == 1:
        r["dlogits==0"] = 0.0 if bool((dlogits.float() == 0).all()) else INF
    return r


def assert_inside(ratios, what):
    print(f"err/bound {what}: "
          + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{what}: outside the bound: {sorted(bad)}"


# ---------------------------------------------------------------------------
# fp32 emulations of the kernels' operation sequences
# ---------------------------------------------------------------------------

def _t32(v):
    return torch.tensor(v, dtype=F32)


def emu_eps(ctr, B, A, mut=None):
    c = torch.tensor(R._i64(int(ctr)), dtype=torch.int64)
    i = torch.arange(B, dtype=torch.int64)[:, None]
    a = torch.arange(A, dtype=torch.int64)[None, :]
    idx = a * B + i if mut == "eps_index" else i * A + a
    h1 = R._sm64(c * 0x100000001 + idx * 2 + (2 if mut == "hash_plus2" else 1))
    h2 = R._sm64(h1)
    u1 = (R._lsr(h1, 40) + 1).to(F32) * 5.9604644775390625e-8
    u2 = (R._lsr(h1 if mut == "u2_from_h1" else h2, 40) + 1).to(F32) \
        * 5.9604644775390625e-8
    return torch.sqrt(-2.0 * torch.log(u1)) \
        * torch.cos(_t32(6.283185307179586) * u2)


def emu_fwd(mu_v, lsr_v, eps, k, mut=None):
    """k_squash_fwd on (possibly strided) views, reading through the base
    buffer as the kernel does: element (i, a) at offset + i ld + a."""
    B, A = mu_v.shape
    i = torch.arange(B)[:, None]
    a = torch.arange(A)[None, :]

    def read(v, ld=None):
        base = v._base if v._base is not None else v
        flat = base.reshape(-1)
        off = v.storage_offset() - base.storage_offset()
        return flat[off + i * (v.stride(0) if ld is None else ld) + a]

    if mut == "swap_halves":
        mu, raw = read(lsr_v), read(mu_v)
    else:
        mu = read(mu_v)
        raw = read(lsr_v, ld=A) if mut == "ls_stride_A" else read(lsr_v)
    k32 = _t32(float(k))
    ls = torch.clamp(raw, -20.0, 2.0)
    s = torch.exp(ls)
    u = mu + s * eps
    t = torch.tanh(u)
    lp = torch.zeros(B)
    for c in range(A):
        e = eps[:, c]
        w = (1.0 - t[:, c] * t[:, c]) + _t32(1e-6)
        lp = lp + ((((-0.5 * e) * e - ls[:, c]) - _t32(0.9189385332046727))
                   - torch.log(k32 * w))
    return dict(act=k32 * t, logp=lp.reshape(B, 1), t=t, ls=ls)


def emu_bwd(ga, gl, raw, ls, eps, t, k, mut=None):
    """k_squash_bwd / k_squash_bwd2: fp32 (du, dlsr) and the joined bf16
    dhead."""
    k32 = _t32(float(k))
    g = gl.reshape(-1, 1)
    if ga.dim() == 3:
        ga = ga[0] if mut == "head0_only" else ga[0] + ga[1]
    omt2 = 1.0 - t * t
    den = omt2 if mut == "no_eps6" else omt2 + _t32(1e-6)
    dlp_du = 2.0 * t * omt2 / den
    s = torch.exp(ls)
    du = (ga * omt2 if mut == "no_k" else ga * k32 * omt2) + g * dlp_du
    m_src = ls if mut == "mask_on_ls" else raw
    one, zero = torch.ones_like(raw), torch.zeros_like(raw)
    mask = torch.where((m_src >= -20.0) & (m_src <= 2.0), one,
                       torch.where(torch.isnan(m_src), m_src, zero))
    dlsr = mask * ((du * eps * s + g) if mut == "plus_g"
                   else (du * eps * s - g))
    halves = [dlsr, du] if mut == "dhead_swapped" else [du, dlsr]
    return du, dlsr, torch.cat(halves, 1).to(BF)


def emu_pool_fwd(logits, z, rep, mut=None):
    Mz, E = logits.shape
    M = Mz * rep
    r = torch.arange(M)
    zrow = r.clamp(max=Mz - 1) if mut == "alpha_row" else r % Mz
    a = logits[zrow]
    mx = torch.zeros(M, 1) if mut == "no_max" \
        else a.max(-1, keepdim=True).values
    ex = torch.exp(a - mx)
    den = torch.zeros(M)
    for e in range(E):
        den = den + ex[:, e]
    al = ex * (1.0 / den).unsqueeze(-1)
    acc = torch.zeros(M, z.shape[2])
    for e in range(E):
        acc = acc + al[:, e:e + 1] * z[e]
    return al[:Mz].contiguous(), acc.to(BF)


def emu_pool_bwd(z, alpha, dz, mut=None):
    E, M, D = z.shape
    dzv = dz.float()
    s = torch.zeros(M, E)
    for e in range(E):
        v = torch.zeros(M, 64)
        v[:, :D] = z[e] * dzv
        o = 32
        while o:                       # the wave's shuffle-down tree
            v = v[:, :o] + v[:, o:2 * o]
            o >>= 1
        s[:, e] = v[:, 0]
    t = torch.zeros(M)
    for e in range(E):
        t = t + alpha[:, e] * s[:, e]
    dzencs = (alpha.t().unsqueeze(-1) * dzv.unsqueeze(0)).to(BF)
    dl = alpha * s if mut == "no_t" else alpha * (s - t.unsqueeze(-1))
    return dzencs, dl.to(BF)


# ---------------------------------------------------------------------------
# (a) the emulation inside every bound, at every GPU shape
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("A", SQ_A)
@pytest.mark.parametrize("B", SQ_B)
def test_emulated_squash_inside_bounds(B, A):
    inp = squash_inputs(B, A)
    for k in SQ_K:
        for layout in SQ_LAYOUTS:
            mu_v, lsr_v = squash_layout(inp["mu"], inp["lsr"], layout)
            out = emu_fwd(mu_v, lsr_v, inp["eps"], k)
            assert_inside(fwd_ratios(inp["mu"], inp["lsr"], inp["eps"], k,
                                     out), f"fwd {B}x{A} k={k} {layout}")
            nan = torch.isnan(out["logp"]).reshape(-1).nonzero().reshape(-1)
            assert nan.tolist() == inp["nan_rows"]
        for ga in (inp["ga"][0], inp["ga"]):
            du, dlsr, dhead = emu_bwd(ga, inp["gl"], inp["lsr"], out["ls"],
                                      inp["eps"], out["t"], k)
            args = (ga, inp["gl"], inp["lsr"], out["ls"], inp["eps"],
                    out["t"], k)
            assert_inside(bwd_ratios(*args, du=du, dlsr=dlsr),
                          f"bwd {B}x{A} k={k} ga{tuple(ga.shape)}")
            assert_inside(bwd_ratios(*args, dhead=dhead),
                          f"bwd2 {B}x{A} k={k} ga{tuple(ga.shape)}")
            if inp["nan_rows"]:
                assert bool(torch.isnan(dhead[2, 2 * A - 1]))   # NaN lsr
                assert bool(torch.isnan(dhead[1, 0]))           # NaN mu


@pytest.mark.parametrize("ctr", COUNTERS)
@pytest.mark.parametrize("B,A", KRNG_SHAPES)
def test_emulated_eps_inside_bound(B, A, ctr):
    assert_inside(eps_ratio(emu_eps(ctr, B, A), ctr), f"eps {B}x{A} c={ctr}")


def test_emulated_eps_2_20_draws():
    """The figure the eps bound's headroom is quoted from: the fp32
    sequence over 2^20 draws at counter 42 stays within a third of it."""
    r = eps_ratio(emu_eps(42, 1 << 20, 1), 42)
    assert_inside(r, "eps 2^20 c=42")
    assert r["eps"] < 0.5


@pytest.mark.parametrize("E", POOL_E)
@pytest.mark.parametrize("D", POOL_D)
def test_emulated_pool_inside_bounds(E, D):
    for Mz in POOL_M:
        for kind in POOL_LOGITS:
            for rep in (1, 2):
                logits, z, _ = pool_inputs(Mz, E, D, rep, kind)
                alpha, pooled = emu_pool_fwd(logits, z, rep)
                assert_inside(pool_fwd_ratios(logits, z, rep, alpha, pooled),
                              f"pool fwd {Mz}x{E}x{D} rep={rep} {kind}")
            for ld, off in ((D, 0), (D + 9, 4)):
                z, alpha, dz_full = pool_bwd_inputs(Mz, E, D, ld, kind)
                dz = dz_full[:, off:off + D]
                dzencs, dl = emu_pool_bwd(z, alpha, dz)
                assert_inside(pool_bwd_ratios(z, alpha, dz, dzencs, dl),
                              f"pool bwd {Mz}x{E}x{D} ld={ld} {kind}")


# ---------------------------------------------------------------------------
# (b) every fault outside a bound
# ---------------------------------------------------------------------------

def _outside(ratios):
    return any(not v <= 1.0 for v in ratios.values())


@pytest.mark.parametrize("mut", ["ls_stride_A", "swap_halves"])
def test_fwd_fault_leaves_a_bound(mut):
    B, A, k = 257, 4, 2.5
    inp = squash_inputs(B, A)
    mu_v, lsr_v = squash_layout(inp["mu"], inp["lsr"], "head_rows")
    args = (inp["mu"], inp["lsr"], inp["eps"], k)
    assert not _outside(fwd_ratios(*args, emu_fwd(mu_v, lsr_v, inp["eps"], k)))
    r = fwd_ratios(*args, emu_fwd(mu_v, lsr_v, inp["eps"], k, mut=mut))
    print(mut, r)
    assert _outside(r)


@pytest.mark.parametrize("mut", ["no_k", "plus_g", "mask_on_ls",
                                 "head0_only", "dhead_swapped", "no_eps6"])
def test_bwd_fault_leaves_a_bound(mut):
    B, A, k = 257, 4, 2.5
    inp = squash_inputs(B, A)
    out = emu_fwd(inp["mu"], inp["lsr"], inp["eps"], k)
    args = (inp["ga"], inp["gl"], inp["lsr"], out["ls"], inp["eps"],
            out["t"], k)
    du, dlsr, dhead = emu_bwd(*args)
    assert not _outside(bwd_ratios(*args, du=du, dlsr=dlsr))
    assert not _outside(bwd_ratios(*args, dhead=dhead))
    du, dlsr, dhead = emu_bwd(*args, mut=mut)
    r = dict(bwd_ratios(*args, du=du, dlsr=dlsr),
             **bwd_ratios(*args, dhead=dhead))
    print(mut, r)
    if mut == "dhead_swapped":
        assert _outside({k_: v for k_, v in r.items() if "dhead" in k_})
    else:
        assert _outside({k_: v for k_, v in r.items() if "dhead" not in k_})
        assert _outside({k_: v for k_, v in r.items() if "dhead" in k_})


@pytest.mark.parametrize("mut", ["eps_index", "hash_plus2", "u2_from_h1"])
def test_eps_fault_leaves_the_bound(mut):
    B, A, ctr = 257, 4, 42
    assert not _outside(eps_ratio(emu_eps(ctr, B, A), ctr))
    assert _outside(eps_ratio(emu_eps(ctr, B, A, mut=mut), ctr))


@pytest.mark.parametrize("mut", ["alpha_row", "no_max"])
def test_pool_fwd_fault_leaves_a_bound(mut):
    Mz, E, D, rep = 5, 6, 50, 2
    logits, z, _ = pool_inputs(Mz, E, D, rep,
                               "big" if mut == "no_max" else "normal")
    assert not _outside(pool_fwd_ratios(logits, z, rep,
                                        *emu_pool_fwd(logits, z, rep)))
    r = pool_fwd_ratios(logits, z, rep, *emu_pool_fwd(logits, z, rep, mut=mut))
    print(mut, r)
    assert _outside(r)


def test_pool_bwd_fault_leaves_the_bound():
    M, E, D = 5, 6, 50
    z, alpha, dz = pool_bwd_inputs(M, E, D, D, "normal")
    assert not _outside(pool_bwd_ratios(z, alpha, dz,
                                        *emu_pool_bwd(z, alpha, dz)))
    r = pool_bwd_ratios(z, alpha, dz, *emu_pool_bwd(z, alpha, dz, mut="no_t"))
    assert r["dlogits"] == INF and r["d_zencs"] == 0.0


def test_nan_log_std_is_visible():
    """torch.clamp keeps a NaN, so the CPU path and the oracle show a
    poisoned log-std head in logp and in both halves of the gradient."""
    inp = squash_inputs(5, 4)
    a, lp, ls = R.squashed_gaussian(inp["mu"], inp["lsr"], inp["eps"], 1.0)
    assert bool(torch.isnan(ls[2, 3])) and bool(torch.isnan(lp[2, 0]))
    o = R.squash_fwd_oracle(inp["mu"], inp["lsr"], inp["eps"], 1.0)
    assert torch.isnan(o["logp"]).reshape(-1).tolist() == \
        [False, True, True, False, False]
    t = o["t"].float()
    du, dlsr, _, _ = R.squash_bwd_oracle(inp["ga"], inp["gl"], inp["lsr"],
                                         o["ls"], inp["eps"], t, 1.0)
    assert bool(torch.isnan(dlsr[2, 3])) and bool(torch.isnan(du[2, 3]))
    assert int(torch.isnan(dlsr).sum()) == 2          # and the NaN mu


# ---------------------------------------------------------------------------
# (c) the allowances
# ---------------------------------------------------------------------------

def _ulps(x32, ref64):
    """Worst error of fp32 ``x32`` against float64 ``ref64`` in ulps of the
    reference (finite, non-zero references only)."""
    ok = torch.isfinite(ref64) & (ref64 != 0)
    ref = ref64[ok]
    _, ex = torch.frexp(ref)                    # |ref| = m 2^ex, m in [.5, 1)
    ulp = torch.ldexp(torch.ones_like(ref), ex - 24)
    return float(((x32[ok].double() - ref).abs() / ulp).max())


def measured_allowances():
    """Worst ulp error of the fp32 torch exp / log / tanh / cos against
    float64, each over the arguments that step sees in these tests."""
    worst = dict(exp=0.0, log=0.0, tanh=0.0, cos=0.0)
    for B in SQ_B:
        for A in SQ_A:
            inp = squash_inputs(B, A)
            out = emu_fwd(inp["mu"], inp["lsr"], inp["eps"], 2.5)
            ls = out["ls"]
            u = inp["mu"] + torch.exp(ls) * inp["eps"]
            w = 2.5 * ((1.0 - out["t"] * out["t"]) + _t32(1e-6))
            for name, fn, x in (("exp", torch.exp, ls), ("tanh", torch.tanh, u),
                                ("log", torch.log, w)):
                worst[name] = max(worst[name], _ulps(fn(x), fn(x.double())))
    c = torch.tensor(42, dtype=torch.int64)
    h1 = R._sm64(c * 0x100000001 + torch.arange(1 << 16) * 2 + 1)
    u1 = (R._lsr(h1, 40) + 1).to(F32) * 5.9604644775390625e-8
    x2 = _t32(6.283185307179586) * \
        ((R._lsr(R._sm64(h1), 40) + 1).to(F32) * 5.9604644775390625e-8)
    worst["log"] = max(worst["log"],
                       _ulps(torch.log(u1), torch.log(u1.double())))
    worst["cos"] = _ulps(torch.cos(x2), torch.cos(x2.double()))
    for Mz in POOL_M:
        logits, _, _ = pool_inputs(Mz, 16, 1, 1, "normal")
        x = logits - logits.max(-1, keepdim=True).values
        worst["exp"] = max(worst["exp"],
                           _ulps(torch.exp(x), torch.exp(x.double())))
    return worst


def test_allowances_are_four_times_the_measured_error():
    m = measured_allowances()
    print("worst ulp error, fp32 torch against float64:", m)
    for name, const in (("exp", R.SQ_E_EXP), ("log", R.SQ_E_LOG),
                        ("tanh", R.SQ_E_TANH), ("cos", R.SQ_E_COS)):
        assert const == 4 * max(1, math.ceil(m[name])), (name, m[name])


# ---------------------------------------------------------------------------
# (d) the eps oracle is standard normal and uncorrelated
# ---------------------------------------------------------------------------

STAT_N = 1 << 20
STAT_COUNTERS = [0, 42, 43, 2 ** 31 - 3]
_DRAWS = {}


def _draw(ctr):
    if ctr not in _DRAWS:
        _DRAWS[ctr] = R.squash_eps_oracle(ctr, STAT_N, 1)[0].reshape(-1)
    return _DRAWS[ctr]


@pytest.mark.parametrize("ctr", STAT_COUNTERS)
def test_eps_oracle_statistics(ctr):
    e = _draw(ctr)
    N = e.numel()
    lim = 4.5 / math.sqrt(N)
    cdf = 0.5 * (1.0 + torch.erf(torch.sort(e).values / math.sqrt(2.0)))
    i = torch.arange(1, N + 1, dtype=torch.float64)
    D = float(torch.maximum((i / N - cdf).max(), (cdf - (i - 1) / N).max()))
    mean, var = float(e.mean()), float(e.var())
    lag1 = float((e[:-1] * e[1:]).mean())
    lag4 = float((e[:-4] * e[4:]).mean())
    print(f"ctr {ctr}: D sqrt(N) {D * math.sqrt(N):.3f} mean {mean:.2e} "
          f"var-1 {var - 1:.2e} lag1 {lag1:.2e} lag4 {lag4:.2e}")
    assert D * math.sqrt(N) < 1.95
    assert abs(mean) < lim and abs(var - 1.0) < 0.01
    assert abs(lag1) < lim and abs(lag4) < lim


def test_eps_oracle_counters_uncorrelated():
    c = float((_draw(42) * _draw(43)).mean())
    print(f"mean(e42 e43) {c:.2e}")
    assert abs(c) < 4.5 / math.sqrt(STAT_N)
