"""k_bf16_chain_fwd_pair: two independent forward chains in one launch.

The pair launch changes no arithmetic and no order, so everything here is
compared with torch.equal:

- the binding against two single-chain launches on the same packed
  weights, over jobs that differ in M, G, input dtypes, concat mode,
  save_acts, widths and layer count;
- the engines with DSAC_PAIR_FWD=1 against DSAC_PAIR_FWD=0, eager and
  captured.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _cdiv(a, b):
    return (a + b - 1) // b


def _job(seed, M, widths, G=1, mode="one", C2=0, save_acts=1, out_f32=1,
         act_last=0):
    """One chain's argument set.  mode: 'one' (single fp32 input), 'ff' /
    'hf' (fp32|fp32 resp. bf16|fp32 column concat, x2 has C2 columns),
    'row' (two fp32 inputs stacked over rows)."""
    from distributed_sac_amd.ops import native
    g = torch.Generator().manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, generator=g).to(DEV)

    K0 = widths[0]
    if mode == "one":
        x1, x2 = rn(M, K0), torch.empty(0, device=DEV)
    elif mode == "row":
        x1, x2 = rn(M // 2 + 1, K0), rn(M - M // 2 - 1, K0)
    else:
        x1, x2 = rn(M, K0 - C2), rn(M, C2)
        if mode == "hf":
            x1 = x1.to(torch.bfloat16)
    ws, bs, wps = [], [], []
    for K, N in zip(widths[:-1], widths[1:]):
        w = (rn(G, N, K) / K ** 0.5).to(torch.bfloat16)
        ws.append(w if G > 1 else w[0].contiguous())
        bs.append(rn(G * N))
        wps.append(torch.empty(G * _cdiv(N, 16) * _cdiv(K, 32) * 512,
                               dtype=torch.bfloat16, device=DEV))
    L = len(ws)
    native().pack_weights_frag(ws, wps, [G] * L, [0] * L)
    return dict(x1=x1, x2=x2, ws=ws, bs=bs, act_last=act_last, G=G,
                out_f32=out_f32, rowcat=1 if mode == "row" else 0,
                save_acts=save_acts, wps=wps)


def _pair_args(j):
    return (j["x1"], j["x2"], j["ws"], j["bs"], j["act_last"], j["G"],
            j["out_f32"], j["rowcat"], j["save_acts"], j["wps"])


def _single(ext, j):
    return ext.mlp_chain_fwd_bf16(
        j["x1"], j["x2"], j["ws"], j["bs"], j["act_last"], j["G"],
        j["out_f32"], 0, j["rowcat"], j["save_acts"], j["wps"])


SHIPPED = [53, 400, 400, 400, 1]

# (job a, job b): kwargs of _job
CASES = {
    # partial last tiles, different tile counts (blocks of b exit early in
    # x), G=2 against G=1 (b's z=1 slice exits), odd 49+4 fp32 concat
    # against the CARE bf16|fp32 concat, widths 40/72 (partial N tiles, a
    # wave with a partial quad, idle waves), heads 1 and 8, 3 and 2 layers
    "ragged": (dict(M=37, widths=[53, 40, 72, 1], G=2, mode="ff", C2=4),
               dict(M=21, widths=[52, 72, 8], G=1, mode="hf", C2=3,
                    out_f32=0, act_last=1)),
    "ragged_swapped": (dict(M=21, widths=[52, 72, 8], G=1, mode="hf", C2=3),
                       dict(M=37, widths=[53, 40, 72, 1], G=2, mode="ff",
                            C2=4)),
    # exactly one tile each
    "one_tile": (dict(M=16, widths=[32, 40, 1], G=2),
                 dict(M=16, widths=[24, 72, 8], G=2, mode="ff", C2=5)),
    # a row-concatenated job next to a no-grad job
    "rowcat": (dict(M=37, widths=[21, 40, 8], mode="row"),
               dict(M=21, widths=[21, 72, 40, 1], G=2, save_acts=0)),
    # the engines' pair: target twin (save_acts=0) + critic twin
    "shipped": (dict(M=37, widths=SHIPPED, G=2, mode="ff", C2=4,
                     save_acts=0),
                dict(M=37, widths=SHIPPED, G=2, mode="ff", C2=4)),
}


@pytest.fixture(scope="module")
def jobs():
    """Each case's two jobs with their single-launch results, computed
    once and left unchanged."""
    from distributed_sac_amd.ops import native
    ext = native()
    out = {}
    for name, (ka, kb) in CASES.items():
        ja, jb = _job(1, **ka), _job(2, **kb)
        out[name] = (ja, jb, _single(ext, ja), _single(ext, jb))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("rm", [1, 2])
@pytest.mark.parametrize("case", list(CASES))
def test_pair_equals_two_single_launches(jobs, case, rm):
    from distributed_sac_amd.ops import native
    ext = native()
    ja, jb, ref_a, ref_b = jobs[case]
    first = ext.mlp_chain_fwd_pair_bf16(*_pair_args(ja), *_pair_args(jb), rm)
    again = ext.mlp_chain_fwd_pair_bf16(*_pair_args(ja), *_pair_args(jb), rm)
    assert len(first) == len(again) == 2
    for j, got, rep, ref in zip((ja, jb), first, again, (ref_a, ref_b)):
        L = len(j["ws"])
        assert len(got) == len(rep) == len(ref) \
            == (2 + L - 1 if j["save_acts"] else 2)
        for i, (t, r2, r) in enumerate(zip(got, rep, ref)):
            if i == 1 and not j["save_acts"]:
                # no-grad job: the bf16 input copy is not made
                assert t.numel() == 0 and r2.numel() == 0
                continue
            assert t.dtype == r.dtype and t.shape == r.shape, (case, i)
            assert torch.equal(t, r), (case, i)
            assert torch.equal(t, r2), (case, i)
        assert got[0].abs().max() > 0


def test_pair_needs_packed_weights(jobs):
    from distributed_sac_amd.ops import native
    ext = native()
    ja, jb, _, _ = jobs["ragged"]

    def call(**over):
        b = dict(jb, **over)
        ext.mlp_chain_fwd_pair_bf16(*_pair_args(ja), *_pair_args(b), 1)

    call()
    with pytest.raises(RuntimeError, match="packed"):
        call(wps=[])
    hole = list(jb["wps"])
    hole[1] = hole[1][:0]
    with pytest.raises(RuntimeError, match="packed"):
        call(wps=hole)
    short = list(jb["wps"])
    short[0] = short[0][:-512].contiguous()
    with pytest.raises(RuntimeError):
        call(wps=short)
    with pytest.raises(RuntimeError):
        call(wps=jb["wps"][:1])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# engines: DSAC_PAIR_FWD=1 against 0
# ---------------------------------------------------------------------------
def _make(case, tmp_path):
    from tests.test_manual_chain import _engine
    if case == "sac":
        from tests.test_engine import small_cfg
        from distributed_sac_amd.algo import SACEngine
        cfg = small_cfg("sac")
        return SACEngine(cfg, "cuda:0", precision="bf16"), cfg
    return _engine(case, tmp_path)


def _count_pair_launches(monkeypatch):
    from distributed_sac_amd.ops import native
    ext = native()
    real = ext.mlp_chain_fwd_pair_bf16
    calls = []

    def counted(*a):
        calls.append(1)
        return real(*a)

    monkeypatch.setattr(ext, "mlp_chain_fwd_pair_bf16", counted)
    return calls


def _assert_same_engines(on, off, fresh):
    from tests.test_manual_chain import _groups
    g1, g0, gf = _groups(on), _groups(off), _groups(fresh)
    for n in g1:
        assert torch.equal(g1[n].flat_data, g0[n].flat_data), n
        # both stepped (a frozen pair would agree trivially)
        assert not torch.equal(gf[n].flat_data, g1[n].flat_data), n
    assert torch.equal(on.target_group.flat_data, off.target_group.flat_data)
    assert torch.equal(on.log_alpha, off.log_alpha)


@pytest.mark.parametrize("case", ["mtsac", "sac", "care_m", "care_orig"])
def test_engine_switch_is_bit_identical(case, tmp_path, monkeypatch):
    from tests.test_engine import make_batch
    monkeypatch.delenv("DSAC_CHAIN", raising=False)
    monkeypatch.delenv("DSAC_PAIR_RM", raising=False)
    calls = _count_pair_launches(monkeypatch)
    engines = {}
    for mode in ("1", "0", "fresh"):
        torch.manual_seed(0)
        engines[mode], cfg = _make(case, tmp_path)
    fresh = engines.pop("fresh")
    for step in range(3):
        batch = {k: v.cuda() for k, v in
                 make_batch(cfg, cfg.batch_size, seed=step).items()}
        eps = [torch.randn(cfg.batch_size, cfg.action_dim, device="cuda")
               for _ in range(2)]
        m = {}
        for mode, e in engines.items():
            monkeypatch.setenv("DSAC_PAIR_FWD", mode)
            before = len(calls)
            e._eps_queue = [t.clone() for t in eps]
            m[mode] = e.update({k: v.clone() for k, v in batch.items()})
            assert len(calls) - before == (1 if mode == "1" else 0)
        assert m["1"].keys() == m["0"].keys()
        for k in m["1"]:
            assert torch.equal(torch.tensor(m["1"][k], dtype=torch.float64),
                               torch.tensor(m["0"][k], dtype=torch.float64)), \
                (step, k)
    torch.cuda.synchronize()
    _assert_same_engines(engines["1"], engines["0"], fresh)


def test_captured_switch_is_bit_identical(monkeypatch):
    from distributed_sac_amd.algo import SACEngine
    from distributed_sac_amd.replay import ShardedReplay
    from tests.test_engine import small_cfg
    monkeypatch.delenv("DSAC_CHAIN", raising=False)
    monkeypatch.delenv("DSAC_PAIR_RM", raising=False)
    calls = _count_pair_launches(monkeypatch)
    cfg = small_cfg("mtsac")
    dev = "cuda:0"

    def run(mode):
        monkeypatch.setenv("DSAC_PAIR_FWD", mode)
        torch.manual_seed(0)
        e = SACEngine(cfg, dev, precision="bf16")
        replay = ShardedReplay(4000, cfg.num_tasks, cfg.mtobs_dim,
                               cfg.action_dim, device=dev)
        for t in range(cfg.num_tasks):
            n = 256
            st = torch.randn(n, cfg.mtobs_dim, device=dev)
            oh = torch.zeros(n, cfg.num_tasks, device=dev)
            oh[:, t] = 1
            st[:, -cfg.num_tasks:] = oh
            replay.shards[t].append(
                st, torch.rand(n, cfg.action_dim, device=dev) * 2 - 1,
                torch.randn(n, 1, device=dev), st.clone(),
                torch.zeros(n, 1, device=dev))
        before = len(calls)
        e.capture(replay, cfg.batch_size, warmup_iters=1, chunk=2)
        # one eager warm-up update + the two captured ones
        assert len(calls) - before == (3 if mode == "1" else 0)
        for _ in range(2):
            m = e.graphed_update()
        torch.cuda.synchronize()
        return e, {k: v.detach().clone() for k, v in m.items()}

    on, m_on = run("1")
    off, m_off = run("0")
    torch.manual_seed(0)
    fresh = SACEngine(cfg, dev, precision="bf16")
    assert m_on.keys() == m_off.keys()
    for k in m_on:
        assert torch.equal(m_on[k], m_off[k]), k
    _assert_same_engines(on, off, fresh)
