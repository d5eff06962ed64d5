"""The float64 TD-target / loss oracles of ops/torch_ref.py (K5-K7), checked
without a GPU (the counterpart of tests/test_squash_oracle.py).

(a) An fp32 torch emulation of each kernel's operation sequence and
    summation order — strided per-thread adds, the xor butterfly, the four
    wave partials, the slots in block order, the alpha gradient's LDS
    columns and per-block task sums — stays inside every bound at every
    shape tests/test_loss_reference.py runs on the GPU.
(b) The same emulation with one of nineteen faults leaves at least one
    bound: the check is sensitive.
(c) A NaN Q-value reaches y, the critic sums and the policy loss.

This module also holds the deterministic inputs and the ``*_ratios``
helpers both test files use.
"""

import pytest
import torch

from distributed_sac_amd.ops import torch_ref as R

F32 = torch.float32
BF = torch.bfloat16
INF = float("inf")
NAN = float("nan")

LOSS_B = [1, 63, 256, 257, 1283, 8192]          # every kernel
LOSS_B_UNFUSED = LOSS_B + [8449]                # 34 strides, 32-block stride
LOSS_TW = [(1, 0), (2, 1), (3, 1), (5, 1), (7, 0), (7, 1), (10, 1), (32, 1)]
LOSS_A = [1, 4, 6]
GAMMA, RS, H_BAR = 0.99, 5.0, -4.0
GSCALE = (0.5, -3.0)
DLA_PAD = 3                                     # dla holds T + 3 floats


def loss_cases():
    """(B, T, use_w, width, A, la_kind): (1, 0) and (10, 1) at every B, all
    of LOSS_TW with and without a state prefix at B = 257 and 1283, A = 1
    and 6 at B = 257, and the 0.3 randn log_alpha once."""
    cases = []
    for B in LOSS_B_UNFUSED:
        cases += [(B, 1, 0, "pre", 4, "range"), (B, 10, 1, "pre", 4, "range")]
    for B in (257, 1283):
        for T, w in LOSS_TW:
            for width in ("pre", "bare"):
                cases.append((B, T, w, width, 4, "range"))
    cases += [(257, 10, 1, "pre", A, "range") for A in (1, 6)]
    cases.append((1283, 10, 1, "pre", 4, "small"))
    return sorted(set(cases))


def case_id(c):
    return "B{}-T{}-w{}-{}-A{}-{}".format(*c)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

ROW_TWO_MAX, ROW_ZERO, ROW_SOFT, ROW_TIE = 5, 9, 17, 23
ROW_NAN_Q1T, ROW_NAN_AQ2 = 1, 2


def loss_inputs(B, T, width="pre", A=4, la_kind="range", nan=False):
    """Deterministic fp32 inputs of one shape.  Unit normals for every Q,
    r, lp and ls, d ~ Bernoulli(0.3), log_alpha uniform in [-4, 2.5] (so
    that exp(-exp(la)) stays normal) or 0.3 randn.  The states are
    ``39 + T`` wide (``pre``) or ``T`` (``bare``: the suffix is the whole
    row); task T - 2 has no rows (T >= 3).  From B = 32 on, row 5 has two
    equal maxima (tasks 0 and T - 1), row 9 an all-zero suffix, row 17 a
    soft one (0.4 at task 0, 0.6 at T - 1), row 23 ``aq1 == aq2``.  With
    ``nan`` and B >= 3, row 1 has a NaN in q1t and row 2 one in aq2."""
    g = torch.Generator().manual_seed(
        7919 * B + 131 * T + 17 * A + (width == "bare") + 2 * (la_kind == "small"))
    W = T + (39 if width == "pre" else 0)
    states = torch.randn(B, W, generator=g)
    tasks = [t for t in range(T) if not (T >= 3 and t == T - 2)]
    task = torch.tensor(tasks)[(torch.arange(B) * 7 + 3) % len(tasks)]
    states[:, W - T:] = torch.nn.functional.one_hot(task, T).float()
    if B >= 32 and T >= 2:
        states[ROW_TWO_MAX, W - T:] = 0.0
        states[ROW_TWO_MAX, W - T] = 1.0
        states[ROW_TWO_MAX, W - 1] = 1.0
        states[ROW_ZERO, W - T:] = 0.0
        states[ROW_SOFT, W - T:] = 0.0
        states[ROW_SOFT, W - T] = 0.4
        states[ROW_SOFT, W - 1] = 0.6
    v = {n: torch.randn(B, 1, generator=g)
         for n in ("r", "q1t", "q2t", "nlp", "q1", "q2", "aq1", "aq2", "lp")}
    v["d"] = (torch.rand(B, 1, generator=g) < 0.3).float()
    v["ls"] = torch.randn(B, A, generator=g)
    if la_kind == "range":
        v["la"] = torch.rand(T, generator=g) * 6.5 - 4.0
    else:
        v["la"] = 0.3 * torch.randn(T, generator=g)
    if B >= 32:
        v["aq2"][ROW_TIE] = v["aq1"][ROW_TIE]
        v["d"][ROW_TWO_MAX] = 0.0       # so that its alpha shows in y
    nan_rows = []
    if nan and B >= 3:
        v["q1t"][ROW_NAN_Q1T] = NAN
        v["aq2"][ROW_NAN_AQ2] = NAN
        nan_rows = [ROW_NAN_Q1T, ROW_NAN_AQ2]
    v.update(states=states.contiguous(), B=B, T=T, A=A, nan_rows=nan_rows,
             gamma=GAMMA, rs=RS, H_bar=H_BAR)
    return v


def nblk_of(B, cap=True):
    n = -(-B // 256)
    return min(n, 32) if cap else n


# ---------------------------------------------------------------------------
# err / bound of a set of outputs (CPU tensors), shared with the GPU tests
# ---------------------------------------------------------------------------

def _worst(out, ref, tol):
    if tuple(out.shape) != tuple(ref.shape):
        return INF
    r = R.bound_ratio(out, ref, tol)
    return float(r.max()) if r.numel() else 0.0


def _vec_ratios(name, out, ref, tol):
    """One ratio per element of a small fp32 output vector."""
    out = out.detach().float().cpu().reshape(-1)[:ref.numel()]
    r = R.bound_ratio(out, ref, tol)
    return {f"{name}{k}": float(r[k]) for k in range(ref.numel())}


def _bits32(x):
    return x.detach().cpu().contiguous().view(torch.int32).long() & 0xFFFFFFFF


def _bits16(x):
    return x.detach().cpu().contiguous().view(torch.int16).long() & 0xFFFF


def _is_plus_zero(x, where):
    bits = _bits16(x) if x.dtype == BF else _bits32(x)
    return 0.0 if bool((bits.reshape(where.shape)[where] == 0).all()) else INF


def td_ratios(inp, y, alpha=None):
    """y of k_td_target_mt / the fused kernel (``alpha`` None) or of
    k_td_target with the per-sample ``alpha`` it was given."""
    if alpha is None:
        ref, tol = R.td_target_oracle(
            inp["r"], inp["d"], inp["q1t"], inp["q2t"], inp["nlp"],
            inp["gamma"], inp["rs"], states=inp["states"],
            log_alpha=inp["la"], T=inp["T"])
    else:
        ref, tol = R.td_target_oracle(
            inp["r"], inp["d"], inp["q1t"], inp["q2t"], inp["nlp"],
            inp["gamma"], inp["rs"], alpha=alpha)
    return {"y": _worst(y.detach().cpu().reshape(-1), ref, tol)}


def critic_ratios(inp, y, use_w, L, out=None, dq=None, wsum=None,
                  gscale=None):
    """Critic loss outputs judged from the fp32 ``y`` they were computed
    from: ``out [>= 7]``, and ``dq [2, B(, 1)]`` (bf16 or fp32) from the
    ``wsum`` the backward was handed."""
    o = R.critic_loss_oracle(inp["q1"], inp["q2"], y, inp["states"],
                             inp["la"], inp["T"], use_w, L, wsum, gscale)
    r = {}
    if out is not None:
        r.update(_vec_ratios("out", out, o["out"], o["tol_out"]))
        if not use_w:
            one = torch.ones(1)
            r["out2==1"] = 0.0 if torch.equal(
                _bits32(out.reshape(-1)[2:3]), _bits32(one)) else INF
    if dq is not None:
        r["dq"] = _worst(dq.detach().cpu().reshape(2, -1), o["dq"],
                         o["tol_dq"])
    return r


def actor_ratios(inp, use_w, L, out=None, daq=None, dlp=None, dla=None,
                 wsum=None, gscale=None, L_dla=None, wsum_in=None):
    """Actor / alpha loss outputs: ``out [8]``; ``daq [2, B(, 1)]`` and
    ``dlp`` from the handed ``wsum``; ``dla`` (T + padding).  ``wsum_in``
    is a normalizer passed in from elsewhere (the critic kernel's
    ``closs[2]``): it is itself judged from log_alpha."""
    T = inp["T"]
    o = R.actor_alpha_loss_oracle(
        inp["aq1"], inp["aq2"], inp["lp"], inp["ls"], inp["states"],
        inp["la"], T, use_w, inp["H_bar"], L, wsum, gscale, L_dla,
        None if dla is None else dla.numel())
    r = {}
    if out is not None:
        r.update(_vec_ratios("out", out, o["out"], o["tol_out"]))
        if not use_w:
            r["out1==1"] = 0.0 if torch.equal(
                _bits32(out.reshape(-1)[1:2]), _bits32(torch.ones(1))) else INF
    if wsum_in is not None and use_w:
        r["wsum_in"] = _worst(torch.tensor([float(wsum_in)], dtype=F32),
                              o["out"][5:6], o["tol_out"][5:6])
    if daq is not None:
        d2 = daq.detach().cpu().reshape(2, -1)
        r["daq"] = _worst(d2, o["daq"], o["tol_daq"])
        r["daq+0"] = _is_plus_zero(d2, o["daq"] == 0)
        if "daq_bits" in o and d2.dtype == BF:
            r["daq bits"] = 0.0 if torch.equal(_bits16(d2),
                                               o["daq_bits"]) else INF
    if dlp is not None:
        r["dlp"] = _worst(dlp.detach().cpu().reshape(-1), o["dlp"],
                          o["tol_dlp"])
    if dla is not None:
        d1 = dla.detach().cpu().reshape(-1)
        r["dla"] = _worst(d1, o["dla"], o["tol_dla"])
        r["dla+0"] = _is_plus_zero(d1, o["tol_dla"] == 0)
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
    return torch.tensor(float(v), dtype=F32)


def fexp(x):
    """__expf: exp2 of the rounded product with log2(e)."""
    return torch.exp2(x * _t32(1.4426950408889634))


def emu_task(states, T, mut=None):
    B, W = states.shape
    ti = torch.zeros(B, dtype=torch.int64)
    if T <= 1:
        return ti
    best = torch.full((B,), -1e30)
    for t in range(T):
        v = states[:, W - T + t]
        m = (v >= best) if mut == "last_max" else (v > best)
        best = torch.where(m, v, best)
        ti = torch.where(m, torch.full_like(ti, t), ti)
    return ti


def emu_weights(la, T):
    a = fexp(la[:T])
    mx = (-a).max()
    smw = fexp(-a - mx)
    den = torch.zeros(())
    for t in range(T):
        den = den + smw[t]
    return smw / den


def _min(a, b, mut):
    return torch.fmin(a, b) if mut == "fmin_drops_nan" else torch.minimum(a, b)


def emu_td(inp, mut=None, alpha=None):
    """k_td_target_mt (td_target_value: one fused multiply-add, two
    products, one sum) or, with ``alpha``, k_td_target uncontracted."""
    f = {n: inp[n].reshape(-1) for n in ("r", "d", "q1t", "q2t", "nlp")}
    qmin = f["q1t"] if mut == "q1_not_min" else _min(f["q1t"], f["q2t"], mut)
    if alpha is None:
        t = emu_task(inp["states"], inp["T"], mut)
        if mut == "alpha_next":
            t = (t + 1) % inp["T"]
        al = fexp(inp["la"][t])
        x = (qmin.double() - al.double() * f["nlp"].double()).float()
    else:
        x = qmin - alpha.reshape(-1) * f["nlp"]
    g, s = _t32(inp["gamma"]), _t32(inp["rs"])
    if mut == "swap_gamma_rs":
        g, s = s, g
    omd = torch.ones_like(f["d"]) if mut == "no_done" else 1.0 - f["d"]
    y = s * f["r"] + (g * omd) * x
    if mut == "drop_last":
        y[-1] = 0.0
    return y


def _butterfly(v):
    """wave_sum64 over the last axis (64 lanes); every lane ends equal."""
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ off]
    return v[..., 0]


def emu_block_sum(terms, nblk, mut=None):
    """The forward reductions: thread (b, tid) adds rows
    ``b 256 + tid + k 256 nblk`` in order, the butterfly, the four wave
    partials left to right, the slots in block order."""
    B = terms.numel()
    per = 256 * nblk
    K = -(-B // per)
    pad = torch.zeros(K * per)
    pad[:B] = terms
    if mut == "drop_last":
        pad[B - 1] = 0.0
    m = pad.reshape(K, nblk, 256)
    if mut == "no_stride":
        m = m[:1]
    acc = torch.zeros(nblk, 256)
    for k in range(m.shape[0]):
        acc = acc + m[k]
    wave = _butterfly(acc.reshape(nblk, 4, 64))
    slot = ((wave[:, 0] + wave[:, 1]) + wave[:, 2]) + wave[:, 3]
    if mut == "stale_slot":
        slot = torch.cat([slot, slot[-1:]])
    r = torch.zeros(())
    for b in range(slot.numel()):
        r = r + slot[b]
    return r


def emu_critic_fwd(inp, y, use_w, nblk, mut=None):
    q1, q2, y = inp["q1"].reshape(-1), inp["q2"].reshape(-1), y.reshape(-1)
    B, T = inp["B"], inp["T"]
    t = emu_task(inp["states"], T, mut)
    w = emu_weights(inp["la"], T)[t] if use_w else torch.ones(B)
    d1, d2 = y - q1, y - q2
    r0 = emu_block_sum((w * d1) * d1, nblk, mut)
    r1 = emu_block_sum((w * d2) * d2, nblk, mut)
    r2 = emu_block_sum(w, nblk, mut)
    wsum = r2 if use_w else _t32(1.0)
    denom = wsum if mut == "no_B" else wsum * _t32(B)
    return torch.stack([r0 / denom, r1 / denom, wsum, r0, r1, r2,
                        (r0 + r1) / denom, _t32(0.0)])


def _coeff(inp, use_w, wsum, mut):
    B, T = inp["B"], inp["T"]
    t = emu_task(inp["states"], T, mut)
    if not use_w:
        c = torch.ones(B)
    elif mut == "no_wsum":
        c = emu_weights(inp["la"], T)[t]
    else:
        c = emu_weights(inp["la"], T)[t] / _t32(wsum)
    return t, (c if mut == "no_B" else c / _t32(B))


def emu_critic_bwd(inp, y, use_w, wsum, gscale=None, mut=None):
    """fp32 ``[2, B]`` (k_critic_loss_bwd with a gscale, else the value
    k_critic_loss_bwd2 / the fused kernel round to bf16)."""
    q1, q2, y = inp["q1"].reshape(-1), inp["q2"].reshape(-1), y.reshape(-1)
    _, c = _coeff(inp, use_w, wsum, mut)
    k = _t32(2.0 if mut == "plus2" else -2.0)
    g = [_t32(1.0)] * 2 if gscale is None else [_t32(v) for v in gscale]
    h = [g[0] * c * k * (y - q1), g[1] * c * k * (y - q2)]
    return torch.stack(h[::-1] if mut == "swap_halves" else h)


def emu_actor_fwd(inp, use_w, nblk, mut=None):
    f = {n: inp[n].reshape(-1) for n in ("aq1", "aq2", "lp")}
    B, T, A = inp["B"], inp["T"], inp["A"]
    t = emu_task(inp["states"], T, mut)
    w = emu_weights(inp["la"], T)[t] if use_w else torch.ones(B)
    la = inp["la"][t]
    al = fexp(inp["la"][(t + 1) % T] if mut == "alpha_next" else la)
    H = _t32(inp["H_bar"])
    qmin = f["aq1"] if mut == "q1_not_min" else _min(f["aq1"], f["aq2"], mut)
    pl = w * -(qmin - al * f["lp"])
    alt = la * ((f["lp"] - H) if mut == "minus_H" else (f["lp"] + H))
    ent = (_t32(R.LOSS_CE) * _t32(A - 1 if mut == "ce_a_minus_1" else A)) \
        .expand(B).clone()
    for a in range(A):
        ent = ent + inp["ls"][:, a]
    r0, r1, r2, r3 = (emu_block_sum(v, nblk, mut) for v in (pl, w, alt, ent))
    wsum = r1 if use_w else _t32(1.0)
    return torch.stack([r0 / (wsum * _t32(B)), wsum, -r2 / _t32(B),
                        r3 / _t32(B), r0, r1, r2, r3])


def emu_actor_bwd(inp, use_w, wsum, dla_mode, gscale=None, mut=None):
    """``(daq [2, B], dlp [B], dla [T + DLA_PAD])`` in fp32.  ``dla_mode``:
    ``agb`` (alpha_grad_block) or ``ws`` (per-block task sums, slots in
    block order)."""
    f = {n: inp[n].reshape(-1) for n in ("aq1", "aq2", "lp")}
    B, T = inp["B"], inp["T"]
    t, c = _coeff(inp, use_w, wsum, mut)
    g = [_t32(1.0)] * 2 if gscale is None else [_t32(v) for v in gscale]
    first = (f["aq1"] < f["aq2"]) if mut == "tie_second" \
        else (f["aq1"] <= f["aq2"])
    v = g[0] * c * -1.0
    z = torch.zeros(B)
    daq = torch.stack([torch.where(first, v, z), torch.where(first, z, v)])
    dlp = g[0] * c if mut == "no_alpha" else g[0] * c * fexp(inp["la"][t])
    H = _t32(inp["H_bar"])
    s = (f["lp"] - H) if mut == "minus_H" else (f["lp"] + H)
    tt = t.clone()
    if mut == "wrong_task":
        tt[B // 2] = (tt[B // 2] + 1) % T
    dla = torch.zeros(T + DLA_PAD)
    if dla_mode == "agb":
        term = g[1] * -s / _t32(B)
        K = -(-B // 256)
        for k in range(T):
            pad = torch.zeros(K * 256)
            pad[:B] = torch.where(tt == k, term, z)
            acc = torch.zeros(256)
            for j in range(K):
                acc = acc + pad[j * 256:(j + 1) * 256]
            c4 = acc.reshape(4, 64)
            dla[k] = dla[k] + _butterfly((c4[0] + c4[1]) + (c4[2] + c4[3]))
    else:
        val = -s / _t32(B)
        nb = -(-B // 256)
        for k in range(T):
            pad = torch.zeros(nb * 256)
            pad[:B] = torch.where(tt == k, val, z)
            c4 = pad.reshape(nb, 4, 64)
            slot = _butterfly((c4[:, 0] + c4[:, 1]) + (c4[:, 2] + c4[:, 3]))
            r = torch.zeros(())
            for b in range(nb):
                r = r + slot[b]
            dla[k] = dla[k] + r
    return daq, dlp, dla


# ---------------------------------------------------------------------------
# the emulated kernels of one case against the oracles
# ---------------------------------------------------------------------------

def emulated_ratios(case, mut=None, nan=False):
    """Every kernel's emulation at one case, each output against its
    oracle: ``{kernel: {output: err / bound}}``.  A fault ``mut`` is applied
    wherever it has a meaning."""
    B, T, use_w, width, A, la_kind = case
    inp = loss_inputs(B, T, width, A, la_kind, nan=nan)
    res = {}
    y = emu_td(inp, mut)
    res["td_mt"] = td_ratios(inp, y)
    y_ok = emu_td(inp)                          # what the losses are given
    if T == 1:
        alpha = fexp(inp["la"][:1]).expand(B).contiguous()
        res["td"] = td_ratios(inp, emu_td(inp, mut, alpha=alpha), alpha=alpha)
    fused = B <= 8192
    for kind, nblk in (("mb", nblk_of(B)), ("1wg", 1)):
        L = R.loss_chain(B, kind, nblk)
        out = emu_critic_fwd(inp, y_ok, use_w, nblk, mut)
        ws = float(out[2])
        res[f"critic_{kind}"] = critic_ratios(
            inp, y_ok, use_w, L, out=out,
            dq=emu_critic_bwd(inp, y_ok, use_w, ws, mut=mut).to(BF), wsum=ws)
        al = emu_actor_fwd(inp, use_w, nblk, mut)
        ws = float(al[1])
        if mut == "wsum_other_la":
            other = dict(inp, la=inp["la"].flip(0) * 0.5)
            ws = float(emu_actor_fwd(other, use_w, nblk)[1])
        mode = "ws" if kind == "mb" else "agb"
        daq, dlp, dla = emu_actor_bwd(inp, use_w, ws, mode, mut=mut)
        res[f"actor_{kind}"] = actor_ratios(
            inp, use_w, L, out=al, daq=daq.to(BF), dlp=dlp, dla=dla, wsum=ws,
            L_dla=R.loss_chain(B, mode, nblk_of(B, cap=False)), wsum_in=ws)
    # the gscale backwards (fp32 outputs, alpha_grad_block)
    ws = float(emu_critic_fwd(inp, y_ok, use_w, 1)[2])
    res["critic_bwd"] = critic_ratios(
        inp, y_ok, use_w, 0, wsum=ws, gscale=GSCALE,
        dq=emu_critic_bwd(inp, y_ok, use_w, ws, GSCALE, mut))
    daq, dlp, dla = emu_actor_bwd(inp, use_w, ws, "agb", GSCALE, mut)
    res["actor_bwd"] = actor_ratios(
        inp, use_w, 0, daq=daq, dlp=dlp, dla=dla, wsum=ws, gscale=GSCALE,
        L_dla=R.loss_chain(B, "agb"))
    if not fused:
        for k in ("critic_mb", "actor_mb"):
            res[k + "_strided"] = res.pop(k)
    return inp, res


def _flat(res):
    return {f"{k}.{o}": v for k, r in res.items() for o, v in r.items()}


@pytest.mark.parametrize("case", loss_cases(), ids=case_id)
def test_emulated_losses_inside_bounds(case):
    _, res = emulated_ratios(case)
    flat = _flat(res)
    assert_inside(flat, case_id(case))
    assert max(flat.values()) < 1.0


# ---------------------------------------------------------------------------
# (b) every fault outside a bound
# ---------------------------------------------------------------------------

FAULT_CASE = (1283, 10, 1, "pre", 4, "range")
FAULTS = {
    # fault: (case, outputs of which at least one must leave its bound)
    "drop_last": (FAULT_CASE, ["td_mt.y", "critic_mb.out3", "actor_mb.out4"]),
    "no_stride": ((8449, 10, 1, "pre", 4, "range"),
                  ["critic_mb_strided.out3", "actor_mb_strided.out7"]),
    "q1_not_min": (FAULT_CASE, ["td_mt.y", "actor_mb.out0"]),
    "no_done": (FAULT_CASE, ["td_mt.y"]),
    "swap_gamma_rs": (FAULT_CASE, ["td_mt.y"]),
    "last_max": (FAULT_CASE, ["td_mt.y", "actor_mb.dlp"]),
    "alpha_next": (FAULT_CASE, ["td_mt.y", "actor_mb.out0"]),
    "no_wsum": (FAULT_CASE, ["critic_mb.dq", "actor_mb.daq"]),
    "no_B": (FAULT_CASE, ["critic_mb.out0", "critic_mb.dq"]),
    "plus2": (FAULT_CASE, ["critic_mb.dq", "critic_bwd.dq"]),
    "swap_halves": (FAULT_CASE, ["critic_mb.dq"]),
    "tie_second": (FAULT_CASE, ["actor_mb.daq", "actor_bwd.daq"]),
    "no_alpha": (FAULT_CASE, ["actor_mb.dlp"]),
    "wrong_task": (FAULT_CASE, ["actor_mb.dla", "actor_1wg.dla"]),
    "minus_H": (FAULT_CASE, ["actor_mb.out2", "actor_mb.dla"]),
    "ce_a_minus_1": (FAULT_CASE, ["actor_mb.out3"]),
    "stale_slot": (FAULT_CASE, ["critic_mb.out3", "actor_mb.out6"]),
    "wsum_other_la": (FAULT_CASE, ["actor_mb.wsum_in"]),
    "fmin_drops_nan": (FAULT_CASE, ["td_mt.y", "actor_mb.out0"]),
}


@pytest.mark.parametrize("mut", sorted(FAULTS))
def test_fault_leaves_a_bound(mut):
    case, expect = FAULTS[mut]
    nan = mut == "fmin_drops_nan"
    good = _flat(emulated_ratios(case, nan=nan)[1])
    assert all(v <= 1.0 for v in good.values())
    bad = _flat(emulated_ratios(case, mut=mut, nan=nan)[1])
    out = sorted(k for k, v in bad.items() if not v <= 1.0)
    print(mut, "leaves:", out)
    for k in expect:
        assert k in out, (mut, k)


def test_nineteen_faults():
    assert len(FAULTS) == 19


# ---------------------------------------------------------------------------
# (c) the task index, and the NaN rule on the CPU path and in the oracles
# ---------------------------------------------------------------------------

def test_task_index_rules():
    inp = loss_inputs(63, 7)
    t = R.loss_task_index(inp["states"], 7)
    assert int(t[ROW_TWO_MAX]) == 0 and int(t[ROW_ZERO]) == 0
    assert int(t[ROW_SOFT]) == 6
    assert not bool((t == 5).any())             # the task without rows
    assert torch.equal(t, emu_task(inp["states"], 7))
    assert torch.equal(R.loss_task_index(inp["states"], 1),
                       torch.zeros(63, dtype=torch.int64))
    bare = loss_inputs(63, 7, "bare")
    assert bare["states"].shape == (63, 7)
    assert torch.equal(R.loss_task_index(bare["states"], 7),
                       emu_task(bare["states"], 7))


@pytest.mark.parametrize("B", [63, 1283])
def test_nan_q_is_visible(B):
    """torch.min keeps a NaN, so the CPU path, the oracles and the
    emulation show a poisoned Q in its own y / dq elements, in the critic
    sums and in the policy loss — and nowhere else."""
    case = (B, 10, 1, "pre", 4, "range")
    inp, res = emulated_ratios(case, nan=True)
    assert_inside(_flat(res), f"NaN rows {case_id(case)}")
    assert inp["nan_rows"] == [ROW_NAN_Q1T, ROW_NAN_AQ2]
    alpha = inp["la"].exp()[R.loss_task_index(inp["states"], 10)]
    y = R.td_target(inp["r"], inp["d"], inp["q1t"], inp["q2t"], inp["nlp"],
                    alpha.reshape(-1, 1), GAMMA, RS).reshape(-1)
    assert torch.isnan(y).nonzero().reshape(-1).tolist() == [ROW_NAN_Q1T]
    y64, _ = R.td_target_oracle(
        inp["r"], inp["d"], inp["q1t"], inp["q2t"], inp["nlp"], GAMMA, RS,
        states=inp["states"], log_alpha=inp["la"], T=10)
    assert torch.isnan(y64).nonzero().reshape(-1).tolist() == [ROW_NAN_Q1T]
    o = R.critic_loss_oracle(inp["q1"], inp["q2"], y64.float(), inp["states"],
                             inp["la"], 10, 1, 10, wsum=1.0)
    assert torch.isnan(o["out"]).tolist() == \
        [True, True, False, True, True, False, True]
    assert torch.isnan(o["dq"]).nonzero().tolist() == \
        [[0, ROW_NAN_Q1T], [1, ROW_NAN_Q1T]]
    a = R.actor_alpha_loss_oracle(
        inp["aq1"], inp["aq2"], inp["lp"], inp["ls"], inp["states"],
        inp["la"], 10, 1, H_BAR, 10, wsum=1.0)
    assert torch.isnan(a["out"]).tolist() == \
        [True, False, False, False, True, False, False, False]
    assert not bool(torch.isnan(a["daq"]).any())
