"""The TD-target and loss kernels (K5-K7: k_td_target, k_td_target_mt,
k_critic_loss_fwd_mb / _1wg / _bwd / _bwd2, k_actor_alpha_loss_fwd_mb /
_1wg / _bwd / _bwd2 and the fused k_critic_td_loss,
k_actor_alpha_loss_fwd_bwd) through their bindings against the float64
oracles of ops/torch_ref.py.  Every element of every output is compared
with its own bound (docs/KERNELS.md "Numerics"); the inputs, the
``*_ratios`` helpers and the proof that the bounds hold for a correct
kernel and break for a faulty one are in tests/test_loss_oracle.py.

y is judged from the inputs; the sums and dq from the y the kernel was
given (for k_critic_td_loss the y td_target_mt returns for the same
inputs); backward coefficients from the wsum the kernel was handed; a
handed-over wsum itself from log_alpha.  The worst err / bound per output
is printed (collected in profiles/loss_reference.md).
"""

import pytest
import torch

from distributed_sac_amd.ops import torch_ref as R
from tests.test_loss_oracle import (
    BF, DLA_PAD, GAMMA, GSCALE, H_BAR, ROW_NAN_AQ2, ROW_NAN_Q1T, RS,
    actor_ratios, assert_inside, case_id, critic_ratios, loss_cases,
    loss_inputs, nblk_of, td_ratios)

pytestmark = pytest.mark.gpu

DEV = "cuda"
TENSORS = ("r", "d", "q1t", "q2t", "nlp", "q1", "q2", "aq1", "aq2", "lp",
           "ls", "states", "la")


def _ext():
    from distributed_sac_amd.ops import native
    return native()


def _dev(inp):
    return {n: inp[n].to(DEV) for n in TENSORS}


def _zeros(n):
    return torch.zeros(n, device=DEV)


def _ticket_reset(ws):
    assert float(ws[0]) == 0.0


def run_case(ext, inp, use_w, tag):
    """Every kernel at one set of inputs, each output inside its bound.
    Returns the outputs the NaN test looks at."""
    B, T = inp["B"], inp["T"]
    d = _dev(inp)
    gs = torch.tensor(GSCALE, device=DEV)
    keep = {}

    # K5
    y = ext.td_target_mt(d["r"], d["d"], d["q1t"], d["q2t"], d["nlp"],
                         d["states"], d["la"], T, GAMMA, RS)
    yc = y.cpu()
    assert_inside(td_ratios(inp, yc), f"td_target_mt {tag}")
    keep["y"] = yc
    if T == 1:
        alpha = d["la"].exp()[:1].expand(B, 1).contiguous()
        y1 = ext.td_target(d["r"], d["d"], d["q1t"], d["q2t"], d["nlp"],
                           alpha, GAMMA, RS)
        assert_inside(td_ratios(inp, y1.cpu(), alpha=alpha.cpu()),
                      f"td_target {tag}")

    # K6 critic, with and without a workspace, and both backwards
    cq = (d["q1"], d["q2"], y, d["states"], d["la"])
    for kind in ("mb", "1wg"):
        nblk = nblk_of(B) if kind == "mb" else 1
        L = R.loss_chain(B, kind, nblk)
        if kind == "mb":
            ws = _zeros(256)
            out = ext.critic_loss_fwd(*cq, T, use_w, ws)[0]
            _ticket_reset(ws)
        else:
            out = ext.critic_loss_fwd(*cq, T, use_w)[0]
        dq = ext.critic_loss_bwd2(*cq, out, T, use_w)
        assert dq.dtype == BF and tuple(dq.shape) == (2, B, 1)
        assert_inside(critic_ratios(inp, yc, use_w, L, out=out.cpu(),
                                    dq=dq.cpu(), wsum=float(out[2])),
                      f"critic_loss_fwd/{kind} + bwd2 {tag}")
        keep[f"closs_{kind}"], keep[f"dq_{kind}"] = out.cpu(), dq.cpu()
    dq1, dq2 = ext.critic_loss_bwd(*cq, out, gs, T, use_w)
    assert_inside(critic_ratios(inp, yc, use_w, 0, wsum=float(out[2]),
                                gscale=GSCALE,
                                dq=torch.stack([dq1.cpu(), dq2.cpu()])),
                  f"critic_loss_bwd {tag}")

    # K6 actor / alpha, with and without workspaces
    aq = (d["aq1"], d["aq2"], d["lp"])
    tail = (d["states"], d["la"])
    nb_all = nblk_of(B, cap=False)
    for kind in ("mb", "1wg"):
        nblk = nblk_of(B) if kind == "mb" else 1
        L = R.loss_chain(B, kind, nblk)
        dla = torch.full((T + DLA_PAD,), 7.0, device=DEV)
        if kind == "mb":
            ws, ws2 = _zeros(256), _zeros(1 + nb_all * T)
            al = ext.actor_alpha_loss_fwd(*aq, d["ls"], *tail, T, use_w,
                                          H_BAR, dla, ws)
            daq, dlp = ext.actor_alpha_loss_bwd2(*aq, *tail, al, dla, T,
                                                 use_w, H_BAR, ws2)
            _ticket_reset(ws)
            _ticket_reset(ws2)
            L_dla = R.loss_chain(B, "ws", nb_all)
        else:
            al = ext.actor_alpha_loss_fwd(*aq, d["ls"], *tail, T, use_w,
                                          H_BAR, dla)
            daq, dlp = ext.actor_alpha_loss_bwd2(*aq, *tail, al, dla, T,
                                                 use_w, H_BAR)
            L_dla = R.loss_chain(B, "agb")
        assert daq.dtype == BF and tuple(daq.shape) == (2, B, 1)
        assert_inside(actor_ratios(inp, use_w, L, out=al.cpu(),
                                   daq=daq.cpu(), dlp=dlp.cpu(),
                                   dla=dla.cpu(), wsum=float(al[1]),
                                   L_dla=L_dla),
                      f"actor_alpha_loss_fwd/{kind} + bwd2 {tag}")
        keep[f"al_{kind}"], keep[f"daq_{kind}"] = al.cpu(), daq.cpu()
    daq1, daq2, dlp, dla = ext.actor_alpha_loss_bwd(*aq, *tail, al, gs, T,
                                                    use_w, H_BAR)
    assert_inside(actor_ratios(inp, use_w, 0, wsum=float(al[1]),
                               gscale=GSCALE, dlp=dlp.cpu(),
                               daq=torch.stack([daq1.cpu(), daq2.cpu()]),
                               dla=dla.cpu()[:T],
                               L_dla=R.loss_chain(B, "agb")),
                  f"actor_alpha_loss_bwd {tag}")

    # the fused tail
    if B > 8192:
        return keep
    nblk = nblk_of(B)
    L = R.loss_chain(B, "mb", nblk)
    ws = _zeros(256)
    closs, dq = ext.critic_td_loss(d["r"], d["d"], d["q1t"], d["q2t"],
                                   d["nlp"], d["q1"], d["q2"], d["states"],
                                   d["la"], T, use_w, GAMMA, RS, ws)
    _ticket_reset(ws)
    assert_inside(critic_ratios(inp, yc, use_w, L, out=closs.cpu(),
                                dq=dq.cpu(), wsum=float(closs[2])),
                  f"critic_td_loss {tag}")
    keep["closs_fused"], keep["dq_fused"] = closs.cpu(), dq.cpu()
    for given in (True, False):
        ws = _zeros(1 + 32 * 4 + nblk * T)
        dla = torch.full((T + DLA_PAD,), 7.0, device=DEV)
        al, daq, dlp = ext.actor_alpha_loss_fwd_bwd(
            *aq, d["ls"], *tail, dla, T, use_w, H_BAR, ws,
            closs[2:3] if given else None)
        _ticket_reset(ws)
        handed = float(closs[2]) if given else float(al[1])
        assert_inside(actor_ratios(inp, use_w, L, out=al.cpu(),
                                   daq=daq.cpu(), dlp=dlp.cpu(),
                                   dla=dla.cpu(), wsum=handed,
                                   L_dla=R.loss_chain(B, "ws", nblk),
                                   wsum_in=handed if given else None),
                      f"actor_alpha_loss_fwd_bwd wsum={given} {tag}")
        keep["al_fused"], keep["daq_fused"] = al.cpu(), daq.cpu()
    return keep


@pytest.mark.parametrize("case", loss_cases(), ids=case_id)
def test_loss_kernels(case):
    B, T, use_w, width, A, la_kind = case
    run_case(_ext(), loss_inputs(B, T, width, A, la_kind), use_w,
             case_id(case))


@pytest.mark.parametrize("case", [(63, 10, 1, "pre", 4, "range"),
                                  (257, 7, 0, "bare", 4, "range"),
                                  (1283, 10, 1, "pre", 4, "range")],
                         ids=case_id)
def test_nan_q_reaches_the_losses(case):
    """A NaN in one target Q and in one actor-side Q: NaN in that row's y,
    in out[0], out[1], out[6] (and the raw sums) of the critic loss, in
    that row's dq elements and in out[0] (and its raw sum) of the actor
    loss; every other element inside its bound (run_case)."""
    B, T, use_w, width, A, la_kind = case
    inp = loss_inputs(B, T, width, A, la_kind, nan=True)
    assert inp["nan_rows"] == [ROW_NAN_Q1T, ROW_NAN_AQ2]
    k = run_case(_ext(), inp, use_w, "NaN " + case_id(case))
    assert torch.isnan(k["y"]).reshape(-1).nonzero().reshape(-1).tolist() \
        == [ROW_NAN_Q1T]
    for v in ("mb", "1wg", "fused"):
        assert torch.isnan(k[f"closs_{v}"][:7]).tolist() == \
            [True, True, False, True, True, False, True]
        assert torch.isnan(k[f"dq_{v}"].float()).reshape(2, B).nonzero() \
            .tolist() == [[0, ROW_NAN_Q1T], [1, ROW_NAN_Q1T]]
        assert torch.isnan(k[f"al_{v}"]).tolist() == \
            [True, False, False, False, True, False, False, False]
        assert not bool(torch.isnan(k[f"daq_{v}"].float()).any())


def test_workspace_reuse():
    """B = 8192, then 1, then 257 on one workspace that is never cleared:
    the last block reads only the slots of its own launch, so every result
    equals the one from a fresh zeroed workspace bit for bit."""
    ext = _ext()
    T, use_w = 10, 1
    sizes = dict(c=256, a=256, b=1 + 32 * T, ct=256, af=1 + 32 * 4 + 32 * T)
    shared = {k: _zeros(n) for k, n in sizes.items()}

    def run(B, ws):
        d = _dev(loss_inputs(B, T))
        y = ext.td_target_mt(d["r"], d["d"], d["q1t"], d["q2t"], d["nlp"],
                             d["states"], d["la"], T, GAMMA, RS)
        aq, tail = (d["aq1"], d["aq2"], d["lp"]), (d["states"], d["la"])
        out = [ext.critic_loss_fwd(d["q1"], d["q2"], y, *tail, T, use_w,
                                   ws["c"])[0][:7]]        # [7] is not written
        dla = torch.full((T + DLA_PAD,), 7.0, device=DEV)
        al = ext.actor_alpha_loss_fwd(*aq, d["ls"], *tail, T, use_w, H_BAR,
                                      dla, ws["a"])
        out += [al, *ext.actor_alpha_loss_bwd2(*aq, *tail, al, dla, T, use_w,
                                               H_BAR, ws["b"]), dla]
        closs, dq = ext.critic_td_loss(d["r"], d["d"], d["q1t"], d["q2t"],
                                       d["nlp"], d["q1"], d["q2"], *tail, T,
                                       use_w, GAMMA, RS, ws["ct"])
        out += [closs[:7], dq]
        dla2 = torch.full((T + DLA_PAD,), 7.0, device=DEV)
        out += [*ext.actor_alpha_loss_fwd_bwd(*aq, d["ls"], *tail, dla2, T,
                                              use_w, H_BAR, ws["af"]), dla2]
        for w in ws.values():
            _ticket_reset(w)
        return [o.cpu() for o in out]

    for B in (8192, 1, 257):
        got = run(B, shared)
        want = run(B, {k: _zeros(n) for k, n in sizes.items()})
        for j, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(g.view(torch.int16) if g.dtype == BF else g,
                               w.view(torch.int16) if w.dtype == BF else w), \
                (B, j)


def test_fast_exp_allowance():
    """__expf measured directly: without weights and at B = 256, dlp is
    alpha / 256 exactly, so dlp 256 is the kernel's alpha bit for bit.
    Over every log_alpha of loss_cases() its error against float64 exp, in
    units of u alpha, stays inside E_fexp(x) = LOSS_E_FEXP + 2 |x|, and
    the constant part is at least four times the worst error (the rule the
    squash allowances follow)."""
    ext = _ext()
    las = torch.cat([loss_inputs(c[0], c[1], c[3], c[4], c[5])["la"]
                     for c in loss_cases()])
    B, T = 256, 32
    worst_e, worst_r = 0.0, 0.0
    for lo in range(0, las.numel(), T):
        la = torch.zeros(T)
        n = min(T, las.numel() - lo)
        la[:n] = las[lo:lo + n]
        task = torch.arange(B) % T
        states = torch.nn.functional.one_hot(task, T).float().to(DEV)
        z = _zeros(B)
        saved = torch.ones(8, device=DEV)
        _, dlp = ext.actor_alpha_loss_bwd2(z, z, z, states, la.to(DEV),
                                           saved, _zeros(T), T, 0, H_BAR)
        alpha = (dlp.cpu().reshape(-1)[:T] * 256.0).double()
        ref = torch.exp(la.double())
        e = (alpha - ref).abs() / (R.SQ_U * ref)
        worst_e = max(worst_e, float(e.max()))
        worst_r = max(worst_r, float((e / (R.loss_e_fexp(la.double())
                                           / R.SQ_U)).max()))
    print(f"__expf over {las.numel()} log_alpha in "
          f"[{float(las.min()):.3f}, {float(las.max()):.3f}]: worst error "
          f"{worst_e:.3f} u alpha, worst error / E_fexp {worst_r:.4f}")
    assert worst_r <= 1.0
    assert 4.0 * worst_e <= R.LOSS_E_FEXP


def test_fused_bindings_refuse_8193_rows():
    ext = _ext()
    B, T = 8193, 10
    d = _dev(loss_inputs(B, T))
    with pytest.raises(RuntimeError):
        ext.critic_td_loss(d["r"], d["d"], d["q1t"], d["q2t"], d["nlp"],
                           d["q1"], d["q2"], d["states"], d["la"], T, 1,
                           GAMMA, RS, _zeros(256))
    with pytest.raises(RuntimeError):
        ext.actor_alpha_loss_fwd_bwd(
            d["aq1"], d["aq2"], d["lp"], d["ls"], d["states"], d["la"],
            _zeros(T), T, 1, H_BAR, _zeros(1 + 32 * 4 + 33 * T))


def test_older_bindings_check_their_arguments():
    """The seven older bindings raise, before any launch, for a column view
    ``x[:, :1]`` of a [B, 2] tensor passed as q1 (they would read it with
    stride 1), for T = 33 (smw[32]) and for a dla longer than the 256
    threads that zero it."""
    ext = _ext()
    B, T = 63, 10
    d = _dev(loss_inputs(B, T))
    col = torch.randn(B, 2, device=DEV)[:, :1]
    assert not col.is_contiguous() and col.numel() == B
    y = _zeros(B)
    saved = torch.ones(8, device=DEV)
    gs = torch.tensor(GSCALE, device=DEV)
    st, la = d["states"], d["la"]
    wide = torch.zeros(B, 40, device=DEV)
    la33 = _zeros(33)

    def calls(q1, states, la, T, dla):
        q2, lp = d["q2"], d["lp"]
        return [
            lambda: ext.td_target_mt(d["r"], d["d"], q1, q2, lp, states, la,
                                     T, GAMMA, RS),
            lambda: ext.critic_loss_fwd(q1, q2, y, states, la, T, 1),
            lambda: ext.critic_loss_fwd(q1, q2, y, states, la, T, 1,
                                        _zeros(256)),
            lambda: ext.critic_loss_bwd(q1, q2, y, states, la, saved, gs, T,
                                        1),
            lambda: ext.critic_loss_bwd2(q1, q2, y, states, la, saved, T, 1),
            lambda: ext.actor_alpha_loss_fwd(q1, q2, lp, d["ls"], states, la,
                                             T, 1, H_BAR, dla),
            lambda: ext.actor_alpha_loss_fwd(q1, q2, lp, d["ls"], states, la,
                                             T, 1, H_BAR, dla, _zeros(256)),
            lambda: ext.actor_alpha_loss_bwd(q1, q2, lp, states, la, saved,
                                             gs, T, 1, H_BAR),
            lambda: ext.actor_alpha_loss_bwd2(q1, q2, lp, states, la, saved,
                                              dla, T, 1, H_BAR),
        ]

    for f in calls(d["q1"], st, la, T, _zeros(T)):        # as they should be
        f()
    torch.cuda.synchronize()
    for f in calls(col, st, la, T, _zeros(T)):
        with pytest.raises(RuntimeError):
            f()
    for f in calls(d["q1"], wide, la33, 33, _zeros(33)):
        with pytest.raises(RuntimeError):
            f()
    for ws in ((), (_zeros(256),)):
        with pytest.raises(RuntimeError):
            ext.actor_alpha_loss_fwd(d["q1"], d["q2"], d["lp"], d["ls"], st,
                                     la, T, 1, H_BAR, _zeros(257), *ws)
    # a strided states view and a short vector are refused too
    with pytest.raises(RuntimeError):
        ext.critic_loss_fwd(d["q1"], d["q2"], y,
                            torch.zeros(B, 80, device=DEV)[:, :49], la, T, 1)
    with pytest.raises(RuntimeError):
        ext.critic_loss_fwd(d["q1"], d["q2"][:B - 1], y, st, la, T, 1)
