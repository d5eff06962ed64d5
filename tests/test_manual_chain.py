"""ops.chain.ManualChain: the one host-side driver of the chain kernels.

- the helper issues exactly what the raw bindings give (bitwise);
- its stored flat-gradient offsets are the .grad views' offsets;
- DSAC_CHAIN=0 (per-layer kernels) tracks DSAC_CHAIN=1 (chain kernels).
"""

import pytest
import torch
import torch.nn as nn

from distributed_sac_amd.ops.flat import FlatParams

WIDTHS = [21, 48, 40, 1]   # no multiple of the 16/32 fragment tile
M = 96                     # not a multiple of the 64-row GEMM tile


def _make_chain(G, dev, arena_off=None):
    """A FlatParams group laid out as the engines lay theirs out (G=2:
    interleaved [Q1.w, Q2.w, Q1.b, Q2.b] per layer), its bf16 mirror and
    the ManualChain over both."""
    from distributed_sac_amd.ops.chain import ManualChain
    g = torch.Generator().manual_seed(G)
    params, w_params, b_params = [], [], []
    for K, N in zip(WIDTHS[:-1], WIDTHS[1:]):
        ws = [nn.Parameter((torch.randn(N, K, generator=g) / K ** 0.5)
                           .to(dev)) for _ in range(G)]
        bs = [nn.Parameter(torch.randn(N, generator=g).to(dev))
              for _ in range(G)]
        params += ws + bs
        w_params.append(ws[0])
        b_params.append(bs[0])
    group = FlatParams(params)
    if arena_off is not None:   # like actor_group inside the shared arena
        shared = torch.zeros(arena_off + group.numel + 3, device=dev)
        group.adopt_grad_arena(shared, arena_off)
    mirror = group.flat_data.to(torch.bfloat16)
    ws16, bs = [], []
    for w, b in zip(w_params, b_params):
        ow = group.offsets[next(i for i, q in enumerate(params) if q is w)]
        ob = group.offsets[next(i for i, q in enumerate(params) if q is b)]
        shape_w = (G, *w.shape) if G > 1 else tuple(w.shape)
        shape_b = (G, *b.shape) if G > 1 else tuple(b.shape)
        ws16.append(mirror[ow:ow + G * w.numel()].view(shape_w))
        bs.append(group.flat_data[ob:ob + G * b.numel()].view(shape_b))
    chain = ManualChain(ws16, bs, G=G, group=group, w_params=w_params,
                        b_params=b_params)
    return chain, group, w_params, b_params


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("arena_off", [None, 5])
def test_stored_grad_offsets(G, arena_off):
    chain, group, w_params, b_params = _make_chain(G, "cpu", arena_off)

    def check():
        base = group.flat_grad.data_ptr()
        for offs, ps in ((chain.w_offs, w_params), (chain.b_offs, b_params)):
            assert len(offs) == len(ps)
            for off, p in zip(offs, ps):
                assert off == (p.grad.data_ptr() - base) // 4

    check()
    group.rebind_grads()
    check()


def _dw_arena_rule(B):
    """SACEngine._dw_arena's split rule."""
    chunk = ((B + 7) // 8 + 63) // 64 * 64
    return (B + chunk - 1) // chunk, chunk


def _cdiv(a, b):
    return (a + b - 1) // b


@pytest.mark.gpu
@pytest.mark.parametrize("G,rowcat", [(1, False), (2, False), (1, True)])
def test_helper_equals_raw_bindings(G, rowcat, monkeypatch):
    """forward / input_grad / backward against the bindings called
    directly, with every argument list written out longhand."""
    from distributed_sac_amd.ops import native
    from distributed_sac_amd.ops.chain import pack_chains
    ext = native()
    monkeypatch.delenv("DSAC_CHAIN", raising=False)
    dev = "cuda"
    chain, group, w_params, b_params = _make_chain(G, dev)
    L = len(WIDTHS) - 1
    ws16, bs = chain.ws16, chain.bs
    torch.manual_seed(3)
    lo = 17
    if rowcat:
        x1 = torch.randn(M // 2, WIDTHS[0], device=dev)
        x2 = torch.randn(M - M // 2, WIDTHS[0], device=dev)
    else:
        x1 = torch.randn(M, lo, device=dev)
        x2 = torch.randn(M, WIDTHS[0] - lo, device=dev)

    def bf(*shape):
        return torch.empty(*shape, dtype=torch.bfloat16, device=dev)

    # ---- the raw sequence ---------------------------------------------
    nk = [(w.numel() // (G * w.shape[-1]), w.shape[-1]) for w in ws16]
    fp = [bf(G * _cdiv(N, 16) * _cdiv(K, 32) * 512) for N, K in nk]
    dxp = [bf(G * _cdiv(K, 16) * _cdiv(N, 32) * 512) for N, K in nk]
    wt = [bf(G, K, N) if G > 1 else bf(K, N) for N, K in nk]
    ext.pack_weights_frag(list(ws16) * 2, fp + dxp, [G] * (2 * L),
                          [0] * L + [1] * L)
    out = ext.mlp_chain_fwd_bf16(x1, x2, list(ws16),
                                 [b.contiguous() for b in bs], 0, G, 1, 0,
                                 1 if rowcat else 0, 1, fp)
    y_ref, acts_ref = out[0], [out[1]] + list(out[2:])

    # ---- the helper ---------------------------------------------------
    pack_chains(ext, [(chain, True, True)])
    y, acts = chain.forward(x1, x2, rowcat=rowcat)
    assert torch.equal(y, y_ref)
    assert len(acts) == len(acts_ref) == L
    for a, r in zip(acts, acts_ref):
        assert torch.equal(a, r)

    base = group.flat_grad.data_ptr()
    w_offs = [(p.grad.data_ptr() - base) // 4 for p in w_params]
    b_offs = [(p.grad.data_ptr() - base) // 4 for p in b_params]
    aflags = [1] * (L - 1) + [0]
    empty_h = bf(0)

    for rows in (None, slice(M // 2, None)):
        Mr = M if rows is None else M - M // 2
        dy = torch.randn(*((G, Mr, 1) if G > 1 else (Mr, 1)),
                         device=dev).to(torch.bfloat16)
        sel = (lambda a: a) if rows is None else (lambda a: a[..., rows, :])
        S, chunk = _dw_arena_rule(Mr)
        youts = [sel(acts_ref[i + 1]) for i in range(L - 1)] + [empty_h]
        if rows is None:
            dx_ref = ext.mlp_chain_dx_bf16(dy, list(wt), youts, WIDTHS[0],
                                           aflags, G, 0, lo, list(dxp))[-1]
            dx = chain.input_grad(dy, acts, lo)
            assert dx.shape == (G, Mr, WIDTHS[0] - lo)
            assert dx.dtype == torch.float32
            assert torch.equal(dx, dx_ref)
        outs = ext.mlp_chain_dx_bf16(dy, list(wt), youts, WIDTHS[0], aflags,
                                     G, 1, 0, list(dxp))
        dx0f = outs[-1]
        dx0_ref = (dx0f[0] + dx0f[1] if G == 2 else dx0f[0]) \
            .to(torch.bfloat16)
        arena_ref = torch.zeros(S, group.numel, device=dev)
        ext.dwdb_grouped_arena(list(outs[:-1]),
                               [sel(acts_ref[i]) for i in range(L)],
                               arena_ref, w_offs, b_offs, G, S, chunk)
        grad_ref = torch.zeros(group.numel, device=dev)
        ext.reduce_arena(arena_ref, grad_ref, S)

        arena = torch.zeros(S, group.numel, device=dev)
        dx0 = chain.backward(dy, acts, arena, S, chunk, rows=rows, dx0_lo=0)
        grad = torch.zeros(group.numel, device=dev)
        ext.reduce_arena(arena, grad, S)
        assert torch.equal(dx0, dx0_ref)
        assert torch.equal(arena, arena_ref)
        assert torch.equal(grad, grad_ref)
        assert grad.abs().max() > 0
        assert chain.backward(dy, acts, arena, S, chunk, rows=rows) is None


def _engine(case, tmp_path):
    from tests.test_care import care_cfg
    from tests.test_engine import small_cfg
    from distributed_sac_amd.algo import CAREEngine, SACEngine
    if case == "mtsac":
        cfg = small_cfg("mtsac")
        return SACEngine(cfg, "cuda:0", precision="bf16"), cfg
    cfg = (care_cfg(tmp_path, modified=True) if case == "care_m"
           else care_cfg(tmp_path, modified=False, num_tasks=1))
    return CAREEngine(cfg, "cuda:0", precision="bf16"), cfg


def _groups(e):
    gs = {"actor": e.actor_group, "critic": e.critic_group}
    if getattr(e, "context_group", None) is not None:
        gs["context"] = e.context_group
    return gs


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["mtsac", "care_m", "care_orig"])
def test_chain_switch_equivalence(case, tmp_path, monkeypatch):
    """DSAC_CHAIN=0 (per-layer kernels) against DSAC_CHAIN=1 (chain
    kernels): 3 updates on shared eps, the bounds of
    test_manual_backward_matches_autograd_bf16.  care_orig: the context
    chain stays on the chain kernels in both modes."""
    from tests.test_engine import make_batch
    engines = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DSAC_CHAIN", mode)
        torch.manual_seed(0)
        engines[mode], cfg = _engine(case, tmp_path)
    for n, g in _groups(engines["1"]).items():
        assert torch.equal(g.flat_data, _groups(engines["0"])[n].flat_data)
    first = None
    for step in range(3):
        batch = {k: v.cuda() for k, v in
                 make_batch(cfg, cfg.batch_size, seed=step).items()}
        eps = [torch.randn(cfg.batch_size, cfg.action_dim, device="cuda")
               for _ in range(2)]
        m = {}
        for mode, e in engines.items():
            monkeypatch.setenv("DSAC_CHAIN", mode)
            e._eps_queue = [t.clone() for t in eps]
            m[mode] = e.update({k: v.clone() for k, v in batch.items()})
        if first is None:
            first = m
    torch.cuda.synchronize()
    dc = abs(first["1"]["critic_loss"] - first["0"]["critic_loss"])
    da = abs(first["1"]["actor_loss"] - first["0"]["actor_loss"])
    dl = (engines["1"].log_alpha - engines["0"].log_alpha).abs().max().item()
    print(f"{case}: first-step |d critic_loss| {dc:.3e} "
          f"|d actor_loss| {da:.3e} |d log_alpha| {dl:.3e}")
    g1, g0 = _groups(engines["1"]), _groups(engines["0"])
    for n in g1:
        d = (g1[n].flat_data - g0[n].flat_data).abs().max().item()
        print(f"{case}: {n} max |d param| {d:.3e}")
    assert dc < 1e-4
    assert da < 1e-4
    for n in g1:
        assert torch.allclose(g1[n].flat_data, g0[n].flat_data,
                              atol=1e-3, rtol=2e-2), n
    assert dl < 1e-3
    # both engines stepped (a frozen pair would agree trivially)
    torch.manual_seed(0)
    monkeypatch.setenv("DSAC_CHAIN", "1")
    fresh, _ = _engine(case, tmp_path)
    for n, g in _groups(fresh).items():
        assert not torch.equal(g.flat_data, g1[n].flat_data), n
        assert not torch.equal(g.flat_data, g0[n].flat_data), n


class _RecordingDP:
    """Stands in for a DataParallelGroup and records what is all-reduced.
    A world-1 group cannot show a missing collective (its all-reduce is
    the identity); the recorded order of buffers can."""
    enabled = True
    world_size = 1

    def __init__(self):
        self.ptrs = []

    def broadcast_params(self, t):
        pass

    def allreduce_grad_(self, t):
        self.ptrs.append(t.data_ptr())


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["mtsac", "care_m", "care_orig"])
def test_allreduce_sequence(case, tmp_path):
    """One update all-reduces exactly [critic flat grad, actor+alpha
    arena], original CARE the context flat grad between the two: eagerly
    and through the segmented data-parallel graphs."""
    from tests.test_engine import make_batch
    from distributed_sac_amd.replay import ShardedReplay
    torch.manual_seed(0)
    e, cfg = _engine(case, tmp_path)
    dp = _RecordingDP()
    e.attach_ddp(dp)
    ctx = _groups(e).get("context")
    assert (ctx is not None) == (case == "care_orig")
    # the actor group's gradient opens the shared actor+alpha arena
    want = [e.critic_group.flat_grad.data_ptr()]
    if ctx is not None:
        want.append(ctx.flat_grad.data_ptr())
    want.append(e.actor_group.flat_grad.data_ptr())
    assert len(set(want)) == len(want)
    assert (e.alpha_group.flat_grad.data_ptr()
            == want[-1] + 4 * e.actor_group.numel)

    batch = {k: v.cuda() for k, v in
             make_batch(cfg, cfg.batch_size, seed=0).items()}
    e.update_tensors(batch)
    assert dp.ptrs == want

    T = cfg.num_tasks
    replay = ShardedReplay(4096, T, cfg.mtobs_dim, cfg.action_dim,
                           device="cuda:0", seed=3)
    for tsk in range(T):
        n = 256
        s = torch.randn(n, cfg.mtobs_dim, device="cuda")
        s[:, -T:] = 0
        s[:, -T + tsk] = 1
        replay.shards[tsk].append(
            s, torch.rand(n, cfg.action_dim, device="cuda") * 2 - 1,
            torch.randn(n, 1, device="cuda"), s.clone(),
            torch.zeros(n, 1, device="cuda"))
    e.capture_dp(replay, cfg.batch_size)
    del dp.ptrs[:]
    m = e.dp_graphed_update()
    torch.cuda.synchronize()
    assert dp.ptrs == want
    assert all(bool(torch.isfinite(v)) for v in m.values())
