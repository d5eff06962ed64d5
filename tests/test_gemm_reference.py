"""Every bf16 MFMA GEMM kernel against the float64 oracle of
ops/torch_ref.py (gemm_oracle / gemm_bound_ratio): the operands are the
kernel's own bf16 inputs, each chain layer is fed the kernel's own saved
output of the layer before, and every element must lie within the bound
derived from the arithmetic — n fp32 additions in any order, one bf16
rounding.  No tolerance here is measured; tests/test_gemm_oracle.py shows
on the CPU that the bound holds for a correct kernel and that one dropped
product, swapped rows, a wrong bias or a stale pad column break it.

Also: pack_weights_frag against its documented layout, and the fp32 ->
bf16 conversion on non-finite inputs.
"""

import pytest
import torch

from distributed_sac_amd.ops import torch_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32

WORST = {}     # (kernel, output class) -> worst err / bound seen


def _check(kernel, cls, out, ref, tol):
    """Every element of ``out`` within its bound; prints the worst ratio
    first (collected in profiles/gemm_reference.md)."""
    r = R.gemm_bound_ratio(out, ref, tol)
    bad = ~torch.isfinite(r)
    worst = float(r[~bad].max()) if bool((~bad).any()) else 0.0
    key = (kernel, cls)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"err/bound {kernel} [{cls}] {tuple(out.shape)}: {worst:.4f}"
          f" violations {int(bad.sum())}")
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(
            f"{kernel} [{cls}]: {int(bad.sum())} of {bad.numel()} elements "
            f"outside the bound, first at {i}: got {float(out[i])!r}, "
            f"ref {float(ref[i])!r}, tol {float(tol[i])!r}")


def _cdiv(a, b):
    return (a + b - 1) // b


def _empty_bf():
    return torch.empty(0, device=DEV, dtype=BF)


# ---------------------------------------------------------------------------
# forward chain
# ---------------------------------------------------------------------------

# x: 'one' fp32 input, 'ff' fp32|fp32 and 'hf' bf16|fp32 column concat (x2
# has C2 columns), 'row' bf16 [9, K0] stacked over fp32 [8, K0]
FWD = {
    # odd K0 on the guarded loader, partial quads, an N = 1 head, a partial
    # last row tile
    "odd_k0": dict(M=37, widths=[53, 40, 72, 1], G=2, x="ff", C2=4),
    # K % 8 != 0; 72 takes the clamped K % 32 tail; bf16 output with ReLU
    "k_tail_bf16_out": dict(M=21, widths=[52, 72, 8], G=1, x="hf", C2=3,
                            out_f32=0, act_last=1),
    # CMAX, two passes over 48 tiles, shrinking widths
    "cmax": dict(M=19, widths=[768, 768, 400, 8], G=1),
    # kbody = 0 (tail only); shrink then grow: stale-column zeroing
    "tail_only": dict(M=33, widths=[24, 16, 200, 1], G=2),
    "six_layers": dict(M=5, widths=[40, 24, 56, 8, 64, 32, 3], G=1),
    "one_tile": dict(M=16, widths=[32, 40, 1], G=2),
    # the row split falls inside a tile
    "rowcat": dict(M=17, widths=[21, 40, 8], G=1, x="row"),
}
DX_CASES = ["odd_k0", "k_tail_bf16_out", "cmax", "tail_only"]
DX0_LO = {"odd_k0": [-1, 0, 49], "k_tail_bf16_out": [-1, 0],
          "cmax": [-1, 0], "tail_only": [-1, 0, 16]}


def _job(seed, M, widths, G=1, x="one", C2=0, out_f32=1, act_last=0):
    from distributed_sac_amd.ops import native
    g = torch.Generator().manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, generator=g).to(DEV)

    K0 = widths[0]
    if x == "one":
        x1, x2 = rn(M, K0), torch.empty(0, device=DEV)
        xcat = x1.to(BF)
    elif x == "row":
        x1, x2 = rn(9, K0).to(BF), rn(M - 9, K0)
        xcat = torch.cat([x1.float(), x2], 0).to(BF)
    else:
        x1, x2 = rn(M, K0 - C2), rn(M, C2)
        if x == "hf":
            x1 = x1.to(BF)
        xcat = torch.cat([x1.float(), x2], 1).to(BF)
    ws, bs, wps, wts, wps_dx = [], [], [], [], []
    for K, N in zip(widths[:-1], widths[1:]):
        w = (rn(G, N, K) / K ** 0.5).to(BF).contiguous()
        ws.append(w if G > 1 else w[0].contiguous())
        bs.append(rn(G * N))
        wts.append(w.transpose(1, 2).contiguous())
        wps.append(torch.empty(G * _cdiv(N, 16) * _cdiv(K, 32) * 512,
                               dtype=BF, device=DEV))
        wps_dx.append(torch.empty(G * _cdiv(K, 16) * _cdiv(N, 32) * 512,
                                  dtype=BF, device=DEV))
    L = len(ws)
    native().pack_weights_frag(ws + ws, wps + wps_dx, [G] * (2 * L),
                               [0] * L + [1] * L)
    return dict(x1=x1, x2=x2, xcat=xcat, ws=ws, bs=bs, wps=wps, wts=wts,
                wps_dx=wps_dx, M=M, widths=widths, G=G, L=L,
                act_last=act_last, out_f32=out_f32,
                rowcat=1 if x == "row" else 0)


def _fwd(ext, j, packed, rm, save_acts):
    return ext.mlp_chain_fwd_bf16(
        j["x1"], j["x2"], j["ws"], j["bs"], j["act_last"], j["G"],
        j["out_f32"], rm, j["rowcat"], save_acts,
        j["wps"] if packed else [])


@pytest.fixture(scope="module")
def jobs():
    """Each forward case with the outputs of one raw-weight launch (the dx
    tests take their masks from it); built once, left unchanged."""
    from distributed_sac_amd.ops import native
    ext = native()
    out = {}
    for i, (name, kw) in enumerate(FWD.items()):
        j = _job(100 + i, **kw)
        j["outs"] = _fwd(ext, j, False, 1, 1)
        out[name] = j
    torch.cuda.synchronize()
    return out


def _check_fwd(kernel, j, outs):
    """out[1] is the exact bf16 input; every saved activation and the
    output within the bound, teacher-forced."""
    G, M, L, widths = j["G"], j["M"], j["L"], j["widths"]
    assert len(outs) == 2 + L - 1
    assert outs[1].dtype == BF and torch.equal(outs[1], j["xcat"])
    assert outs[0].dtype == (F32 if j["out_f32"] else BF)
    x = outs[1].reshape(1, M, widths[0]).expand(G, M, widths[0])
    for li in range(L):
        K, N = widths[li], widths[li + 1]
        last = li == L - 1
        got = outs[0] if last else outs[2 + li]
        assert got.shape == ((M, N) if G == 1 else (G, M, N))
        if not last:
            assert got.dtype == BF
        got = got.reshape(G, M, N)
        ref, tol = R.gemm_oracle(
            x, j["ws"][li].reshape(G, N, K), j["bs"][li].reshape(G, N),
            relu=(not last) or bool(j["act_last"]))
        cls = ("fp32 output" if j["out_f32"] else "bf16 output") if last \
            else "bf16 activation"
        _check(kernel, cls, got, ref, tol)
        x = got


@pytest.mark.parametrize("rm", [1, 2])
@pytest.mark.parametrize("packed", [0, 1])
@pytest.mark.parametrize("case", list(FWD))
def test_chain_fwd(jobs, case, packed, rm):
    from distributed_sac_amd.ops import native
    ext = native()
    j = jobs[case]
    outs = _fwd(ext, j, packed, rm, 1)
    _check_fwd(f"k_bf16_chain_fwd<{rm}> {'packed' if packed else 'raw'}",
               j, outs)
    nosave = _fwd(ext, j, packed, rm, 0)
    assert len(nosave) == 2
    assert torch.equal(nosave[0], outs[0])
    assert torch.equal(nosave[1], outs[1])


@pytest.mark.parametrize("rm", [1, 2])
def test_chain_fwd_pair(jobs, rm):
    from distributed_sac_amd.ops import native
    ext = native()
    ja, jb = jobs["odd_k0"], jobs["k_tail_bf16_out"]

    def args(j):
        return (j["x1"], j["x2"], j["ws"], j["bs"], j["act_last"], j["G"],
                j["out_f32"], j["rowcat"], 1, j["wps"])

    oa, ob = ext.mlp_chain_fwd_pair_bf16(*args(ja), *args(jb), rm)
    _check_fwd(f"k_bf16_chain_fwd_pair<{rm}>", ja, oa)
    _check_fwd(f"k_bf16_chain_fwd_pair<{rm}>", jb, ob)


# ---------------------------------------------------------------------------
# dx chain
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("packed", [0, 1])
@pytest.mark.parametrize("case,dx0_lo", [(c, lo) for c in DX_CASES
                                         for lo in DX0_LO[c]])
def test_chain_dx(jobs, case, dx0_lo, packed):
    from distributed_sac_amd.ops import native
    ext = native()
    j = jobs[case]
    G, M, L, widths = j["G"], j["M"], j["L"], j["widths"]
    K0, NL = widths[0], widths[-1]
    outs = j["outs"]
    youts = [outs[2 + i] for i in range(L - 1)]
    youts.append(outs[0] if j["act_last"] else _empty_bf())
    flags = [1] * (L - 1) + [j["act_last"]]
    gen = torch.Generator().manual_seed(7)
    dy_last = torch.randn(G, M, NL, generator=gen).to(DEV).to(BF)
    res = ext.mlp_chain_dx_bf16(
        dy_last if G > 1 else dy_last[0].contiguous(), j["wts"], youts, K0,
        flags, G, 1, dx0_lo, j["wps_dx"] if packed else [])
    assert len(res) == L + (1 if dx0_lo >= 0 else 0)
    dys = res[:L]
    kernel = f"k_bf16_chain_dx {'packed' if packed else 'raw'}"
    # entry layer: dy_last, masked by the output's ReLU where it has one
    want = dy_last
    if j["act_last"]:
        want = torch.where(youts[-1].reshape(G, M, NL) != 0, dy_last,
                           torch.zeros_like(dy_last))
    assert dys[L - 1].shape == (G, M, NL) and dys[L - 1].dtype == BF
    assert torch.equal(dys[L - 1], want)
    for li in range(L - 2, -1, -1):
        K, N = widths[li + 1], widths[li + 2]   # dy_li [M, K] = dy [M, N] W
        assert dys[li].shape == (G, M, K) and dys[li].dtype == BF
        mask = youts[li].reshape(G, M, K) != 0
        assert bool((dys[li][~mask] == 0).all())
        ref, tol = R.gemm_oracle(dys[li + 1], j["wts"][li + 1], mask=mask)
        _check(kernel, "bf16 dy", dys[li], ref, tol)
    if dx0_lo >= 0:
        dx0 = res[L]
        assert dx0.dtype == F32 and dx0.shape == (G, M, K0 - dx0_lo)
        ref, tol = R.gemm_oracle(dys[0], j["wts"][0][:, dx0_lo:, :])
        _check(kernel, "fp32 dx0", dx0, ref, tol)


# ---------------------------------------------------------------------------
# split-K dW/db into the phase arena
# ---------------------------------------------------------------------------

ARENA = dict(M=130, chunk=64, S=3, G=2,
             layers=[(40, 53), (72, 40), (1, 72), (400, 24)])   # (N, K)


@pytest.fixture(scope="module")
def arena_case():
    M, G = ARENA["M"], ARENA["G"]
    gen = torch.Generator().manual_seed(11)
    dys, xs, w_offs, b_offs = [], [], [], []
    off = 5
    for i, (N, K) in enumerate(ARENA["layers"]):
        dys.append(torch.randn(G, M, N, generator=gen).to(DEV).to(BF))
        # the first layer's input is shared by both groups
        xs.append(torch.randn(*((M, K) if i == 0 else (G, M, K)),
                              generator=gen).to(DEV).to(BF))
        w_offs.append(off)
        off += G * N * K
        b_offs.append(off)
        off += G * N + 7 + i          # a gap before the next layer
    return dict(dys=dys, xs=xs, w_offs=w_offs, b_offs=b_offs,
                numel=off + 3)


def _check_arena(kernel, c, arena, out):
    M, G, S, chunk = ARENA["M"], ARENA["G"], ARENA["S"], ARENA["chunk"]
    inside = torch.zeros(c["numel"], dtype=torch.bool, device=DEV)
    for i, (N, K) in enumerate(ARENA["layers"]):
        inside[c["w_offs"][i]:c["b_offs"][i] + G * N] = True
    assert arena.shape == (S, c["numel"])
    assert bool(torch.isfinite(arena[:, inside]).all()), \
        "a slot inside a layer's range was not written"
    assert bool(torch.isnan(arena[:, ~inside]).all()), \
        "a slot outside every layer's range was written"
    assert bool(torch.isfinite(out[inside]).all())
    assert bool(torch.isnan(out[~inside]).all())
    for i, (N, K) in enumerate(ARENA["layers"]):
        dyT = c["dys"][i].transpose(1, 2)                     # [G, N, M]
        x = c["xs"][i]
        xT = (x if x.dim() == 3 else x.expand(G, M, K)).transpose(1, 2)
        ones = torch.ones(G, 1, M, device=DEV)
        wo, bo = c["w_offs"][i], c["b_offs"][i]
        for s in range(S):
            rows = slice(s * chunk, min(M, (s + 1) * chunk))
            ref, tol = R.gemm_oracle(dyT[..., rows], xT[..., rows])
            _check(kernel, "fp32 dW partial",
                   arena[s, wo:wo + G * N * K].reshape(G, N, K), ref, tol)
            ref, tol = R.gemm_oracle(dyT[..., rows], ones[..., rows])
            _check(kernel, "fp32 db partial",
                   arena[s, bo:bo + G * N].reshape(G, N, 1), ref, tol)
        ref, tol = R.gemm_oracle(dyT, xT, n=M + S)
        _check(kernel + " + k_reduce_arena", "fp32 dW",
               out[wo:wo + G * N * K].reshape(G, N, K), ref, tol)
        ref, tol = R.gemm_oracle(dyT, ones, n=M + S)
        _check(kernel + " + k_reduce_arena", "fp32 db",
               out[bo:bo + G * N].reshape(G, N, 1), ref, tol)


def _nan_arena(c):
    S = ARENA["S"]
    return (torch.full((S, c["numel"]), float("nan"), device=DEV),
            torch.full((c["numel"],), float("nan"), device=DEV))


def _reduce_layers(ext, c, arena, out):
    G, S = ARENA["G"], ARENA["S"]
    for i, (N, K) in enumerate(ARENA["layers"]):
        ext.reduce_arena(arena, out, S, c["w_offs"][i],
                         c["b_offs"][i] + G * N)


def test_dwdb_grouped_arena(arena_case):
    from distributed_sac_amd.ops import native
    ext = native()
    c = arena_case
    arena, out = _nan_arena(c)
    ext.dwdb_grouped_arena(c["dys"], c["xs"], arena, c["w_offs"],
                           c["b_offs"], ARENA["G"], ARENA["S"],
                           ARENA["chunk"])
    _reduce_layers(ext, c, arena, out)
    _check_arena("k_bf16_dwdb_grouped", c, arena, out)


def test_linear_bwd_dwdb_arena(arena_case):
    from distributed_sac_amd.ops import native
    ext = native()
    c = arena_case
    arena, out = _nan_arena(c)
    for i in range(len(ARENA["layers"])):
        ext.linear_bwd_dwdb_arena(c["dys"][i], c["xs"][i], c["dys"][i], 0,
                                  ARENA["G"], arena, c["w_offs"][i],
                                  c["b_offs"][i], ARENA["S"],
                                  ARENA["chunk"], 0)
    _reduce_layers(ext, c, arena, out)
    _check_arena("k_bf16_dwdb_splitk (arena)", c, arena, out)


# ---------------------------------------------------------------------------
# per-layer kernels
# ---------------------------------------------------------------------------

PER_LAYER = [(100, 7, 3), (37, 40, 53), (70, 400, 72)]   # M, N, K


def _layer(M, N, K, G):
    gen = torch.Generator().manual_seed(1000 * M + G)

    def rn(*shape):
        return torch.randn(*shape, generator=gen).to(DEV)

    x = rn(G, M, K).to(BF)
    w = (rn(G, N, K) / K ** 0.5).to(BF)
    b = rn(G, N)
    dy = rn(G, M, N).to(BF)
    yout = rn(G, M, N).relu().to(BF)     # about half the entries are 0
    return x, w, b, dy, yout


def _g(t, G):
    """The bindings' convention: no group dim when G == 1."""
    return t if G > 1 else t[0].contiguous()


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("M,N,K", PER_LAYER)
def test_linear_act_fwd(M, N, K, G):
    from distributed_sac_amd.ops import native
    ext = native()
    x, w, b, _, _ = _layer(M, N, K, G)
    ref, tol = R.gemm_oracle(x, w, b, relu=True)
    for out_f32 in (1, 0):
        y = ext.linear_act_fwd_bf16(_g(x, G), w, b, 1, G, out_f32)
        assert y.dtype == (F32 if out_f32 else BF)
        assert y.shape == ((M, N) if G == 1 else (G, M, N))
        _check("k_bf16_fwd", "fp32 output" if out_f32 else "bf16 output",
               y.reshape(G, M, N), ref, tol)
    if G > 1:
        # one input shared by the groups
        y = ext.linear_act_fwd_bf16(x[0].contiguous(), w, b, 1, G, 1)
        ref, tol = R.gemm_oracle(x[:1].expand(G, M, K), w, b, relu=True)
        _check("k_bf16_fwd", "fp32 output", y, ref, tol)


@pytest.mark.parametrize("reduce", [0, 1])
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("M,N,K", PER_LAYER)
def test_linear_bwd_dx(M, N, K, G, reduce):
    from distributed_sac_amd.ops import native
    ext = native()
    _, w, _, dy, yout = _layer(M, N, K, G)
    dx = ext.linear_bwd_dx_bf16(_g(dy, G), w, _g(yout, G), 1, G, reduce)
    assert dx.dtype == BF
    dym = torch.where(yout != 0, dy, torch.zeros_like(dy))
    if reduce or G == 1:
        assert dx.shape == (M, K)
        # one sum over the G * N terms of all groups
        ref, tol = R.gemm_oracle(
            dym.permute(1, 0, 2).reshape(1, M, G * N),
            w.permute(2, 0, 1).reshape(1, K, G * N))
        _check("k_bf16_dx", "bf16 dx, summed over groups" if G > 1
               else "bf16 dx", dx.reshape(1, M, K), ref, tol)
    else:
        assert dx.shape == (G, M, K)
        ref, tol = R.gemm_oracle(dym, w.transpose(1, 2))
        _check("k_bf16_dx", "bf16 dx", dx, ref, tol)


def _dwdb_splits(M, N, K, G):
    """The number of split-K partials linear_bwd_dwdb_bf16 picks."""
    S = max(1, 512 // max(1, _cdiv(N, 64) * _cdiv(K, 64) * G))
    S = min(S, _cdiv(M, 64))
    chunk = _cdiv(_cdiv(M, S), 64) * 64
    return _cdiv(M, chunk)


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("M,N,K", PER_LAYER)
def test_linear_bwd_dwdb(M, N, K, G):
    from distributed_sac_amd.ops import native
    ext = native()
    x, _, _, dy, yout = _layer(M, N, K, G)
    dw, db = ext.linear_bwd_dwdb_bf16(_g(dy, G), _g(x, G), _g(yout, G), 1, G)
    assert dw.dtype == F32 and db.dtype == F32
    assert dw.shape == ((N, K) if G == 1 else (G, N, K))
    assert db.shape == ((N,) if G == 1 else (G, N))
    dymT = torch.where(yout != 0, dy, torch.zeros_like(dy)).transpose(1, 2)
    n = M + _dwdb_splits(M, N, K, G)
    ref, tol = R.gemm_oracle(dymT, x.transpose(1, 2), n=n)
    _check("k_bf16_dwdb_splitk + k_reduce_dwdb", "fp32 dW",
           dw.reshape(G, N, K), ref, tol)
    ref, tol = R.gemm_oracle(dymT, torch.ones(G, 1, M, device=DEV), n=n)
    _check("k_bf16_dwdb_splitk + k_reduce_dwdb", "fp32 db",
           db.reshape(G, N, 1), ref, tol)


# ---------------------------------------------------------------------------
# narrow forward
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("out_f32", [1, 0])
@pytest.mark.parametrize("G,K0,M", [(6, 39, 70), (1, 768, 65)])
def test_mlp_narrow_fwd(G, K0, M, out_f32):
    from distributed_sac_amd.ops import native
    ext = native()
    widths = [K0, 64, 17, 50]
    gen = torch.Generator().manual_seed(K0)

    def rn(*shape):
        return torch.randn(*shape, generator=gen).to(DEV)

    x = rn(G, M, K0).to(BF)
    ws = [(rn(G, N, K) / K ** 0.5).to(BF)
          for K, N in zip(widths[:-1], widths[1:])]
    bs = [rn(G, N) for N in widths[1:]]
    act_last = 0 if out_f32 else 1
    outs = ext.mlp_narrow_fwd_bf16(_g(x, G), ws, bs, G, act_last, out_f32, 1)
    assert len(outs) == 3
    cur = x
    for li in range(3):
        last = li == 2
        got = outs[0] if last else outs[1 + li]
        N = widths[li + 1]
        assert got.shape == ((M, N) if G == 1 else (G, M, N))
        assert got.dtype == (F32 if last and out_f32 else BF)
        got = got.reshape(G, M, N)
        ref, tol = R.gemm_oracle(cur, ws[li], bs[li],
                                 relu=(not last) or bool(act_last))
        cls = ("fp32 output" if out_f32 else "bf16 output") if last \
            else "bf16 activation"
        _check("k_bf16_mlp_narrow", cls, got, ref, tol)
        cur = got


# ---------------------------------------------------------------------------
# pack_weights_frag
# ---------------------------------------------------------------------------

def test_pack_weights_frag_layout():
    """Both modes of three shapes in one launch, against the layout
    documented above k_bf16_pack_frag built by index arithmetic; the
    buffers start out non-zero, so the out-of-range zeros are written."""
    from distributed_sac_amd.ops import native
    ext = native()
    gen = torch.Generator().manual_seed(5)
    ws, ps, Gs, dxs, want = [], [], [], [], []
    for G, N, K in [(2, 40, 53), (1, 1, 72), (2, 72, 8)]:
        w = (torch.randn(G, N, K, generator=gen) + 3.0).to(DEV).to(BF)
        assert bool((w != 0).all())
        for dx in (0, 1):
            ref = R.pack_frag_ref(w, G, bool(dx))
            rows, cols = (K, N) if dx else (N, K)
            assert ref.numel() == G * _cdiv(rows, 16) * _cdiv(cols, 32) * 512
            assert int((ref != 0).sum()) == w.numel()
            ws.append(w)
            ps.append(torch.full((ref.numel(),), 7.0, dtype=BF, device=DEV))
            Gs.append(G)
            dxs.append(dx)
            want.append(ref)
    ext.pack_weights_frag(ws, ps, Gs, dxs)
    for i, (p, ref) in enumerate(zip(ps, want)):
        assert torch.equal(p, ref), i


# ---------------------------------------------------------------------------
# fp32 -> bf16 on non-finite inputs
# ---------------------------------------------------------------------------

NONFINITE = [0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF,   # lost before
             0x7F80FFFF, 0x7FBFFFFF, 0xFFBF8000,               # other NaNs
             0x7FC00000, 0xFFC00000,                           # quiet NaNs
             0x7F800000, 0xFF800000,                           # +-Inf
             0x7F7FFFFF, 0xFF7FFFFF,          # largest finite: rounds to Inf
             0x3F808000, 0x3F818000, 0x00000001, 0x80000000, 0x3F800000]


def _from_bits(bits):
    u = torch.tensor(bits, dtype=torch.int64)
    return (u - ((u >> 31) << 32)).to(torch.int32).to(DEV).view(F32)


def _check_cast(src, dst):
    """isnan in <=> isnan out; +-Inf and every finite value as torch's own
    round-to-nearest-even cast and as the bits of the documented formula
    (the payload of a NaN is the hardware's choice)."""
    assert dst.dtype == BF and dst.shape == src.shape
    nan = torch.isnan(src)
    assert torch.equal(torch.isnan(dst), nan)
    assert torch.equal(dst[~nan].view(torch.int16),
                       src[~nan].to(BF).view(torch.int16))
    inf = torch.isinf(src)
    assert torch.equal(dst[inf].float(), src[inf])
    want = R.f32_to_bf16_bits(src.view(torch.int32).to(torch.int64))
    got = dst.view(torch.int16).to(torch.int64) & 0xFFFF
    assert torch.equal(got[~nan], want[~nan])


def test_nonfinite_cast_kernel():
    from distributed_sac_amd.ops import native
    ext = native()
    src = _from_bits(NONFINITE)
    assert int(torch.isnan(src).sum()) == 9
    dst = torch.zeros(src.numel(), dtype=BF, device=DEV)
    ext.f32_to_bf16_(src, dst)
    _check_cast(src, dst)


def test_cast_kernel_every_exponent():
    """Every sign, exponent (denormals included) and upper mantissa,
    crossed with the ties, their neighbours and both ends of the 16 bits
    that are rounded away."""
    from distributed_sac_amd.ops import native
    ext = native()
    lo = torch.tensor([0, 1, 0x4000, 0x7FFF, 0x8000, 0x8001, 0xC000, 0xFFFE,
                       0xFFFF], dtype=torch.int32, device=DEV)
    hi = torch.arange(1 << 16, dtype=torch.int32, device=DEV) << 16
    src = (hi[:, None] | lo[None, :]).reshape(-1).view(F32)
    dst = torch.zeros(src.numel(), dtype=BF, device=DEV)
    ext.f32_to_bf16_(src, dst)
    _check_cast(src, dst)


def test_nonfinite_chain_fwd_input(jobs):
    from distributed_sac_amd.ops import native
    ext = native()
    j = dict(jobs["one_tile"])
    x = j["x1"].clone()
    x.view(-1)[:len(NONFINITE)] = _from_bits(NONFINITE)
    j["x1"] = x
    for packed in (0, 1):
        outs = _fwd(ext, j, packed, 1, 1)
        _check_cast(x, outs[1])


def test_nonfinite_adam_bf16_mirror():
    """A poisoned gradient must poison the bf16 mirror exactly where it
    poisons the fp32 master."""
    from distributed_sac_amd.ops.flat import FlatParams, FusedAdam
    torch.manual_seed(0)
    p = torch.nn.Parameter(torch.randn(1000, device=DEV))
    group = FlatParams([p])
    opt = FusedAdam(group, lr=1e-3)
    opt.bf16_mirror = torch.zeros(group.numel, dtype=BF, device=DEV)
    group.flat_grad.copy_(torch.randn(group.numel, device=DEV))
    bad = _from_bits(NONFINITE[:11])
    group.flat_grad[:bad.numel()] = bad
    opt.step()
    torch.cuda.synchronize()
    master, mirror = group.flat_data, opt.bf16_mirror
    nan = torch.isnan(master)
    # a NaN or an infinite gradient leaves a NaN parameter
    assert bool(nan[:bad.numel()].all())
    assert int(nan.sum()) == bad.numel()
    _check_cast(master, mirror)
