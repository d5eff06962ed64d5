"""The float64 GEMM oracle of ops/torch_ref.py, checked without a GPU.

(a) A torch emulation of a kernel — bf16-valued fp32 operands, fp32
    accumulation in 32-wide k chunks (one MFMA step each), then bias, ReLU,
    mask and one bf16 (or no) rounding — must satisfy the oracle's bound on
    every element of every shape tests/test_gemm_reference.py runs on the
    GPU.
(b) The same emulation with one product dropped, two weight rows swapped,
    the other group's bias, or one stale non-zero pad column must violate
    the bound in every tensor the fault can reach: the check is sensitive.
(c) The fp32 -> bf16 conversion the kernels use: the NaN-safe formula
    equals the former one on every finite and infinite input, equals
    torch's own cast there, and keeps every NaN a NaN.
"""

import pytest
import torch

from distributed_sac_amd.ops import torch_ref as R

BF = torch.bfloat16

# M, widths, G, out_f32, act_last — the forward chains of the GPU test
FWD = [
    (37, [53, 40, 72, 1], 2, 1, 0),
    (21, [52, 72, 8], 1, 0, 1),
    (19, [768, 768, 400, 8], 1, 1, 0),
    (33, [24, 16, 200, 1], 2, 1, 0),
    (5, [40, 24, 56, 8, 64, 32, 3], 1, 1, 0),
    (16, [32, 40, 1], 2, 1, 0),
    (17, [21, 40, 8], 1, 1, 0),           # the row-concatenated job
]
NARROW = [(6, 39, 70), (1, 768, 65)]      # G, K0, M; widths K0,64,17,50
DWDB = dict(M=130, chunk=64, S=3, G=2,
            layers=[(40, 53), (72, 40), (1, 72), (400, 24)])
PER_LAYER = [(100, 7, 3), (37, 40, 53), (70, 400, 72)]   # M, N, K


def _bf(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def emulate(a, w, bias=None, relu=False, mask=None, out_dtype=BF,
            drop=None, stale=None):
    """One GEMM as a kernel computes it.  a [G, M, K], w [G, N, K] hold
    bf16 values; fp32 accumulation chunk by chunk.  ``drop = (g, r, c, k)``
    leaves one product out; ``stale = v`` adds a pad column holding ``v``
    in every row against the last weight column (what a clamped k-tail
    load multiplies a stale LDS column with)."""
    a32, w32 = a.float(), w.float()
    if stale is not None:
        a32 = torch.cat([a32, torch.full_like(a32[..., :1], stale)], -1)
        w32 = torch.cat([w32, w32[..., -1:]], -1)

    def run(x):
        acc = torch.zeros(x.shape[0], x.shape[1], w32.shape[1])
        for k0 in range(0, x.shape[-1], 32):
            acc = acc + x[..., k0:k0 + 32] @ \
                w32[..., k0:k0 + 32].transpose(-1, -2)
        return acc

    acc = run(a32)
    if drop is not None:
        g, r, c, k = drop
        a_mod = a32.clone()
        a_mod[g, r, k] = 0.0
        acc[g, r, c] = run(a_mod)[g, r, c]
    if bias is not None:
        acc = acc + bias.float().unsqueeze(-2)
    if relu:
        acc = acc.clamp(min=0.0)
    if mask is not None:
        acc = torch.where(mask, acc, torch.zeros_like(acc))
    return acc.to(out_dtype)


def _gemm(name, a, w, bias=None, relu=False, mask=None, out_dtype=BF,
          n=None):
    return dict(name=name, a=a, w=w, bias=bias, relu=relu, mask=mask,
                out_dtype=out_dtype, n=n)


def _run(c, **fault):
    return emulate(c["a"], c["w"], c["bias"], c["relu"], c["mask"],
                   c["out_dtype"], **fault)


def _build_cases():
    """Every GEMM of every listed shape, teacher-forced: a chain layer's
    input is the emulation's own bf16 output of the layer before."""
    g = torch.Generator().manual_seed(1234)
    cases = []
    for ci, (M, widths, G, out_f32, act_last) in enumerate(FWD):
        x = _bf(g, 1, M, widths[0]).expand(G, M, widths[0]).contiguous()
        L = len(widths) - 1
        ws, youts = [], []
        for li, (K, N) in enumerate(zip(widths[:-1], widths[1:])):
            last = li == L - 1
            w = _bf(g, G, N, K, scale=K ** -0.5)
            b = torch.randn(G, N, generator=g)
            c = _gemm(f"fwd{ci}.l{li}", x, w, b,
                      relu=(not last) or bool(act_last),
                      out_dtype=torch.float32 if last and out_f32 else BF)
            cases.append(c)
            ws.append(w)
            if not last:
                x = _run(c)
                youts.append(x)
        if ci >= 4:
            continue
        # the dx chain of the first four shapes
        dy = _bf(g, G, M, widths[-1])
        if act_last:
            dy = torch.where(_run(cases[-1]) != 0, dy, torch.zeros_like(dy))
        for li in range(L - 1, 0, -1):
            c = _gemm(f"dx{ci}.l{li}", dy, ws[li].transpose(1, 2),
                      mask=youts[li - 1] != 0)
            cases.append(c)
            dy = _run(c)
        cases.append(_gemm(f"dx{ci}.dx0", dy, ws[0].transpose(1, 2),
                           out_dtype=torch.float32))
    for G, K0, M in NARROW:
        widths = [K0, 64, 17, 50]
        x = _bf(g, G, M, K0)
        for li, (K, N) in enumerate(zip(widths[:-1], widths[1:])):
            last = li == 2
            c = _gemm(f"narrow{K0}.l{li}", x, _bf(g, G, N, K,
                                                 scale=K ** -0.5),
                      torch.randn(G, N, generator=g), relu=not last,
                      out_dtype=torch.float32 if last else BF)
            cases.append(c)
            if not last:
                x = _run(c)
    M, S, chunk, G = DWDB["M"], DWDB["S"], DWDB["chunk"], DWDB["G"]
    for N, K in DWDB["layers"]:
        dy, x = _bf(g, G, M, N), _bf(g, G, M, K)
        for s in range(S):
            rows = slice(s * chunk, min(M, (s + 1) * chunk))
            cases.append(_gemm(f"dwdb{N}x{K}.s{s}",
                               dy[:, rows].transpose(1, 2),
                               x[:, rows].transpose(1, 2),
                               out_dtype=torch.float32))
            cases.append(_gemm(f"db{N}.s{s}", dy[:, rows].transpose(1, 2),
                               torch.ones(G, 1, rows.stop - rows.start),
                               out_dtype=torch.float32))
    for M, N, K in PER_LAYER:
        for G in (1, 2):
            x, w = _bf(g, G, M, K), _bf(g, G, N, K, scale=K ** -0.5)
            b = torch.randn(G, N, generator=g)
            for od in (torch.float32, BF):
                cases.append(_gemm(f"lin{M}.{N}.{K}.g{G}.{od}", x, w, b,
                                   relu=True, out_dtype=od))
            dy = _bf(g, G, M, N)
            cases.append(_gemm(f"lindx{M}.{N}.{K}.g{G}", dy,
                               w.transpose(1, 2)))
            # group-reduced dx: one sum over all G * N terms
            cases.append(_gemm(
                f"lindxsum{M}.{N}.{K}.g{G}",
                dy.transpose(0, 1).reshape(1, M, G * N),
                w.transpose(1, 2).transpose(0, 1).reshape(1, K, G * N)))
            cases.append(_gemm(f"lindw{M}.{N}.{K}.g{G}", dy.transpose(1, 2),
                               x.transpose(1, 2), out_dtype=torch.float32))
    return cases


@pytest.fixture(scope="module")
def cases():
    return _build_cases()


def _ratio(c, out, n=None):
    ref, tol = R.gemm_oracle(c["a"], c["w"], c["bias"], c["relu"],
                             c["mask"], n if n is not None else c["n"])
    return R.gemm_bound_ratio(out, ref, tol)


def test_emulated_kernel_within_bounds(cases):
    worst = {torch.float32: 0.0, BF: 0.0}
    total = 0
    for c in cases:
        r = _ratio(c, _run(c))
        assert torch.isfinite(r).all(), \
            (c["name"], int((~torch.isfinite(r)).sum()))
        worst[c["out_dtype"]] = max(worst[c["out_dtype"]], float(r.max()))
        total += r.numel()
    print(f"{len(cases)} GEMMs, {total} elements, worst err/bound: "
          f"fp32 {worst[torch.float32]:.3f} bf16 {worst[BF]:.3f}")
    assert worst[BF] <= 1.0 and worst[torch.float32] <= 1.0


def test_split_k_sum_within_bounds():
    """Partials folded in fp32, n = rows + partials."""
    g = torch.Generator().manual_seed(7)
    M, S, chunk, G = DWDB["M"], DWDB["S"], DWDB["chunk"], DWDB["G"]
    for N, K in DWDB["layers"]:
        dy, x = _bf(g, G, M, N), _bf(g, G, M, K)
        acc = torch.zeros(G, N, K)
        for s in range(S):
            rows = slice(s * chunk, min(M, (s + 1) * chunk))
            acc = acc + emulate(dy[:, rows].transpose(1, 2),
                                x[:, rows].transpose(1, 2),
                                out_dtype=torch.float32)
        ref, tol = R.gemm_oracle(dy.transpose(1, 2), x.transpose(1, 2),
                                 n=M + S)
        assert torch.isfinite(R.gemm_bound_ratio(acc, ref, tol)).all()


def _live(c):
    """Elements whose pre-activation value is positive (or that have no
    ReLU) and that no mask forces to zero: where a fault can show."""
    pre, _ = R.gemm_oracle(c["a"], c["w"], c["bias"])
    live = pre > 0 if c["relu"] else torch.ones_like(pre, dtype=torch.bool)
    if c["mask"] is not None:
        live = live & c["mask"]
    return pre, live


def test_dropped_product_is_caught(cases):
    for c in cases:
        pre, live = _live(c)
        # the largest product of a live element that stays live without it
        prod = c["a"].double().unsqueeze(2) * c["w"].double().unsqueeze(1)
        keep = live.unsqueeze(-1)
        if c["relu"]:
            keep = keep & ((pre.unsqueeze(-1) - prod) > 0)
        score = torch.where(keep, prod.abs(), torch.zeros_like(prod))
        idx = int(score.argmax())
        assert float(score.reshape(-1)[idx]) > 0, c["name"]
        gi, r, col, k = (int(v) for v in
                         torch.unravel_index(torch.tensor(idx), score.shape))
        bad = _ratio(c, _run(c, drop=(gi, r, col, k)))
        assert torch.isinf(bad[gi, r, col]), c["name"]
        assert int(torch.isinf(bad).sum()) == 1, c["name"]


def test_swapped_weight_rows_are_caught(cases):
    n = 0
    for c in cases:
        N = c["w"].shape[1]
        if N < 2:
            continue              # a single output column has no neighbour
        sw = dict(c)
        perm = torch.arange(N)
        perm[0], perm[N - 1] = N - 1, 0
        sw["w"] = c["w"][:, perm]
        bad = _ratio(c, _run(sw))
        assert torch.isinf(bad[..., 0]).any() or \
            torch.isinf(bad[..., N - 1]).any(), c["name"]
        assert not torch.isinf(bad[..., 1:N - 1]).any(), c["name"]
        n += 1
    assert n > 40


def test_other_groups_bias_is_caught(cases):
    n = 0
    for c in cases:
        if c["bias"] is None or c["a"].shape[0] < 2:
            continue
        sw = dict(c)
        sw["bias"] = c["bias"].flip(0)
        assert torch.isinf(_ratio(c, _run(sw))).any(), c["name"]
        n += 1
    assert n > 10


def test_stale_pad_column_is_caught(cases):
    for c in cases:
        # a stale activation of the layer before: any non-zero bf16
        bad = _ratio(c, _run(c, stale=0.5))
        _, live = _live(c)
        reach = live & (c["w"][..., -1] != 0).unsqueeze(1)
        assert reach.any(), c["name"]
        assert torch.isinf(bad).any(), c["name"]


# ---------------------------------------------------------------------------
# fp32 -> bf16
# ---------------------------------------------------------------------------

def _old_bits(u):
    """The former conversion: the RNE add with no NaN case."""
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF) >> 16


def _patterns():
    """Every sign and exponent, every upper mantissa, crossed with a dense
    sample of the 16 bits that are rounded away: the ties, their
    neighbours, both ends and a stride."""
    lo = set(range(0, 0x10000, 251))
    for centre in (0, 0x4000, 0x7FFF, 0x8000, 0x8001, 0xC000, 0xFFFF):
        lo.update(v for v in range(centre - 3, centre + 4)
                  if 0 <= v <= 0xFFFF)
    hi = torch.arange(1 << 16, dtype=torch.int64)[:, None] << 16
    return (hi + torch.tensor(sorted(lo), dtype=torch.int64)[None, :]) \
        .reshape(-1)


def test_bf16_conversion_formula():
    u = _patterns()
    assert u.numel() > 15_000_000
    new = R.f32_to_bf16_bits(u)
    is_nan = (u & 0x7FFFFFFF) > 0x7F800000
    # bit-identical to the former formula off the NaNs
    assert torch.equal(new[~is_nan], _old_bits(u)[~is_nan])
    # and to torch's own round-to-nearest-even cast
    f = (u - ((u >> 31) << 32)).to(torch.int32).view(torch.float32)
    tb = f.to(BF).view(torch.int16).to(torch.int64) & 0xFFFF
    assert torch.equal(new[~is_nan], tb[~is_nan])
    # a NaN stays a NaN, quiet, with its sign
    nn = new[is_nan]
    assert bool(((nn & 0x7FFF) > 0x7F80).all())
    assert bool(((nn & 0x0040) != 0).all())
    assert torch.equal(nn >> 15, u[is_nan] >> 31)
    # the former formula lost some of them: the finding this fixes
    old = _old_bits(u)[is_nan]
    assert bool(((old & 0x7FFF) <= 0x7F80).any())


def test_bf16_conversion_named_patterns():
    u = torch.tensor([0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF,
                      0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000],
                     dtype=torch.int64)
    assert R.f32_to_bf16_bits(u).tolist() == [
        0x7FC0, 0xFFC0, 0x7FFF, 0xFFFF, 0x7FC0, 0xFFC0, 0x7F80, 0xFF80]
    assert _old_bits(u).tolist()[:4] == [0x7F80, 0xFF80, 0x8000, 0x0000]


def test_pack_frag_ref_layout():
    """The index arithmetic of pack_frag_ref against the documented
    formula, element by element, on a small matrix."""
    G, N, K = 2, 19, 37
    w = torch.arange(G * N * K, dtype=torch.float32).reshape(G, N, K) + 1
    for dx in (False, True):
        src = w.transpose(1, 2) if dx else w
        rows, cols = src.shape[1], src.shape[2]
        NT, KS = (rows + 15) // 16, (cols + 31) // 32
        p = R.pack_frag_ref(w, G, dx).reshape(G, NT, KS, 64, 8)
        for g_ in range(G):
            for t in range(NT):
                for ks in range(KS):
                    for l in (0, 1, 15, 16, 37, 63):
                        for j in (0, 3, 7):
                            r = t * 16 + (l & 15)
                            c = ks * 32 + (l >> 4) * 8 + j
                            want = float(src[g_, r, c]) \
                                if r < rows and c < cols else 0.0
                            assert float(p[g_, t, ks, l, j]) == want
