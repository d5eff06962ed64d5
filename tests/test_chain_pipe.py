"""The re-shaped packed k-loop of the bf16 chain kernels (DSAC_CHAIN_PIPE).

k_bf16_chain_fwd_pipe / k_bf16_chain_dx_pipe give the columns to other
waves and load further ahead than the 8-wave quad kernels, but every output
element is still one accumulator that receives its k-steps in ascending
order.  So everything here is compared with torch.equal:

- the forward and the dx binding with pipe=1 against pipe=0 on the same
  packed weights: the shipped critic and actor shapes, layers of 1..8 and
  24 k-steps (every prologue / tail length of the pipeline, layers shorter
  than the look-ahead included), 48 tiles, and a single tile;
- a flagship-shaped engine with DSAC_CHAIN_PIPE=1 against 0, eager and
  captured.

The pair launch keeps its 8-wave quad instantiation and has no selector.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
PIPE = 1   # the shipped variant

# kwargs of tests.test_pair_fwd._job
FWD_CASES = {
    # the shipped critic: 25 tiles, a lone last tile, idle waves
    "critic": dict(M=17, widths=[53, 400, 400, 400, 1], G=2, mode="ff",
                   C2=4),
    # the shipped actor
    "actor": dict(M=37, widths=[49, 400, 400, 400, 8], G=1, mode="row"),
    # layers of 2, 1, 2, 3, 4 and of 2, 5, 6, 7, 8 k-steps
    "ks_1_4": dict(M=21, widths=[53, 32, 64, 96, 128, 1], G=2),
    "ks_5_8": dict(M=16, widths=[40, 160, 192, 224, 256, 8], G=1,
                   out_f32=0, act_last=1),
    # CMAX: 24 k-steps, 48 tiles
    "cmax": dict(M=16, widths=[768, 768, 16]),
    # one tile, every other wave idle, one partial row tile
    "tiny": dict(M=5, widths=[32, 16, 1]),
}


def _cdiv(a, b):
    return (a + b - 1) // b


def _fwd(ext, j, pipe):
    return ext.mlp_chain_fwd_bf16(
        j["x1"], j["x2"], j["ws"], j["bs"], j["act_last"], j["G"],
        j["out_f32"], 0, j["rowcat"], j["save_acts"], j["wps"], pipe)


def _dx_job(j, kw, seed):
    """The dx-side arguments over the forward job's weights: W^T, the dx
    pack, random bf16 dy_last, random post-ReLU masks with exact zeros."""
    from distributed_sac_amd.ops import native
    g = torch.Generator().manual_seed(seed)
    G, M, widths = j["G"], kw["M"], kw["widths"]
    lead = (G,) if G > 1 else ()
    wts, wps = [], []
    for w, K, N in zip(j["ws"], widths[:-1], widths[1:]):
        wts.append(w.transpose(-1, -2).contiguous())
        wps.append(torch.empty(G * _cdiv(K, 16) * _cdiv(N, 32) * 512,
                               dtype=torch.bfloat16, device=DEV))
    L = len(wts)
    native().pack_weights_frag(j["ws"], wps, [G] * L, [1] * L)
    youts = [torch.randn(*lead, M, N, generator=g).clamp_min(0)
             .to(torch.bfloat16).to(DEV) for N in widths[1:-1]]
    for y in youts:
        assert (y == 0).any() and (y != 0).any()
    youts.append(torch.empty(0, dtype=torch.bfloat16, device=DEV))
    dy = torch.randn(*lead, M, widths[-1], generator=g) \
        .to(torch.bfloat16).to(DEV)
    return dict(dy=dy, wts=wts, youts=youts, K0=widths[0],
                acts=[1] * (L - 1) + [0], G=G, wps=wps)


def _dx(ext, d, save_dys, dx0_lo, pipe):
    return ext.mlp_chain_dx_bf16(d["dy"], d["wts"], d["youts"], d["K0"],
                                 d["acts"], d["G"], save_dys, dx0_lo,
                                 d["wps"], pipe)


@pytest.fixture(scope="module")
def jobs():
    """Each case's forward and dx arguments with the pipe=0 results,
    computed once and left unchanged."""
    from distributed_sac_amd.ops import native
    from tests.test_pair_fwd import _job
    ext = native()
    out = {}
    for i, (name, kw) in enumerate(FWD_CASES.items()):
        j = _job(10 + i, **kw)
        d = _dx_job(j, kw, 100 + i)
        out[name] = (j, _fwd(ext, j, 0), d, _dx(ext, d, 1, -1, 0))
    torch.cuda.synchronize()
    return out


def _assert_same(got, ref, what):
    assert len(got) == len(ref), what
    for i, (t, r) in enumerate(zip(got, ref)):
        assert t.dtype == r.dtype and t.shape == r.shape, (what, i)
        assert torch.equal(t, r), (what, i)


@pytest.mark.parametrize("case", list(FWD_CASES))
def test_forward_equals_quad_kernel(jobs, case):
    from distributed_sac_amd.ops import native
    j, ref, _, _ = jobs[case]
    got = _fwd(native(), j, PIPE)
    assert len(got) == 2 + len(j["ws"]) - 1   # y, x_bf16, every hidden act
    _assert_same(got, ref, case)
    assert got[0].float().abs().max() > 0


@pytest.mark.parametrize("case", list(FWD_CASES))
def test_dx_equals_quad_kernel(jobs, case):
    from distributed_sac_amd.ops import native
    _, _, d, ref = jobs[case]
    got = _dx(native(), d, 1, -1, PIPE)
    assert len(got) == len(d["wts"])          # every masked dy
    _assert_same(got, ref, case)
    assert got[0].float().abs().max() > 0


def test_dx_input_gradient_equals_quad_kernel(jobs):
    from distributed_sac_amd.ops import native
    ext = native()
    _, _, d, _ = jobs["critic"]
    lo = d["K0"] - 4
    ref = _dx(ext, d, 1, lo, 0)
    got = _dx(ext, d, 1, lo, PIPE)
    assert got[-1].dtype == torch.float32
    assert got[-1].shape == (d["G"], 17, 4)
    _assert_same(got, ref, "critic dx0")
    assert got[-1].abs().max() > 0
    # the dx-only walk of the actor step: no masked dy is returned
    ref = _dx(ext, d, 0, lo, 0)
    got = _dx(ext, d, 0, lo, PIPE)
    assert torch.equal(got[-1], ref[-1])


def test_selector_and_packed_weights_are_checked(jobs):
    from distributed_sac_amd.ops import native
    ext = native()
    j, _, d, _ = jobs["tiny"]
    for bad in (-1, 2):
        with pytest.raises(RuntimeError, match="pipe"):
            _fwd(ext, j, bad)
        with pytest.raises(RuntimeError, match="pipe"):
            _dx(ext, d, 1, -1, bad)
    with pytest.raises(RuntimeError, match="packed"):
        _fwd(ext, dict(j, wps=[]), PIPE)
    with pytest.raises(RuntimeError, match="packed"):
        _dx(ext, dict(d, wps=[]), 1, -1, PIPE)
    # the quad kernels still take raw weights
    _assert_same(_fwd(ext, dict(j, wps=[]), 0), jobs["tiny"][1], "raw fwd")
    _assert_same(_dx(ext, dict(d, wps=[]), 1, -1, 0), jobs["tiny"][3],
                 "raw dx")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# engine: DSAC_CHAIN_PIPE=1 against 0, flagship shapes at B = 40, T = 10
# ---------------------------------------------------------------------------
def _flagship_cfg():
    from distributed_sac_amd.config import load_variant
    cfg = load_variant("mtsac")
    assert cfg.num_tasks == 10
    cfg.batch_size = 40
    return cfg


def _count_launches(monkeypatch):
    """Records the pipe argument of every forward / dx binding call."""
    from distributed_sac_amd.ops import native
    ext = native()
    seen = []
    for name in ("mlp_chain_fwd_bf16", "mlp_chain_dx_bf16"):
        real = getattr(ext, name)

        def counted(*a, _real=real):
            seen.append(a[-1])
            return _real(*a)

        monkeypatch.setattr(ext, name, counted)
    return seen


def _assert_same_engines(on, off, fresh):
    for n in ("actor_group", "critic_group", "target_group"):
        a, b = getattr(on, n).flat_data, getattr(off, n).flat_data
        assert torch.equal(a, b), n
        if n != "target_group":
            # both stepped (a frozen pair would agree trivially)
            assert not torch.equal(a, getattr(fresh, n).flat_data), n
    assert torch.equal(on.log_alpha, off.log_alpha)


def test_engine_switch_is_bit_identical(monkeypatch):
    from distributed_sac_amd.algo import SACEngine
    from tests.test_engine import make_batch
    monkeypatch.delenv("DSAC_CHAIN", raising=False)
    seen = _count_launches(monkeypatch)
    cfg = _flagship_cfg()
    engines = {}
    for mode in ("1", "0", "fresh"):
        torch.manual_seed(0)
        engines[mode] = SACEngine(cfg, "cuda:0", precision="bf16")
    fresh = engines.pop("fresh")
    for step in range(3):
        batch = {k: v.cuda() for k, v in
                 make_batch(cfg, cfg.batch_size, seed=step).items()}
        eps = [torch.randn(cfg.batch_size, cfg.action_dim, device="cuda")
               for _ in range(2)]
        m = {}
        for mode, e in engines.items():
            monkeypatch.setenv("DSAC_CHAIN_PIPE", mode)
            before = len(seen)
            e._eps_queue = [t.clone() for t in eps]
            m[mode] = e.update({k: v.clone() for k, v in batch.items()})
            assert len(seen) > before
            assert set(seen[before:]) == {int(mode)}
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
    monkeypatch.delenv("DSAC_CHAIN", raising=False)
    cfg = _flagship_cfg()
    dev = "cuda:0"

    def run(mode):
        monkeypatch.setenv("DSAC_CHAIN_PIPE", mode)
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
        e.capture(replay, cfg.batch_size, warmup_iters=1, chunk=2)
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
