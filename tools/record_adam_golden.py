"""Golden record of the Adam/Polyak kernel family, for a refactor that
must not move a bit.

Seven cases, three consecutive steps each, through the extension's
bindings only (adam_step_, adam_step_dev_, adam_prolog_many,
adam_step_multi_, adam_step_clip_, polyak_), so the same file runs on any
commit that keeps those signatures:

    python tools/record_adam_golden.py      # on the commit to pin, on a GPU

writes tests/golden/adam_family.npz: the inputs (drawn from a seeded CPU
generator, stored under ``in/``) and every array the kernels wrote, after
every step (under ``out/``).  tests/test_adam_golden.py replays ``in/``
through ``run_cases`` and compares with ``out/`` bit for bit.
"""

import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "adam_family.npz")
LR, B1, B2, EPS = 3e-4, 0.9, 0.999, 1e-8
STEPS = 3
S = 7                       # arena rows summed; the arena has one spare row
N_DEV = (1, 257, 1000)      # one thread, two blocks, partial last block
N_MULTI = (1, 257, 1000)
N_CLIP = (1000, 300, 10)
NP, TAU = 513, 0.005
LRS4 = (3e-4, 1e-3, 5e-5, 2e-4)
CLIP_MAX = (10.0, 100.0, float("inf"))   # clipped, under, guard only


def make_inputs():
    gen = torch.Generator().manual_seed(20261021)

    def r(*shape):
        return torch.randn(*shape, generator=gen)

    inp = {"arena": r(S + 1, 1000), "src": r(STEPS, NP), "tgt": r(NP),
           "c1/p": r(1000), "c1/g": r(STEPS, 1000), "c3/p": r(1000),
           "c5/p0": r(1000), "c5/p1": r(10), "c5/g1": r(STEPS, 10)}
    for n in N_DEV:
        inp[f"c2_{n}/p"], inp[f"c2_{n}/g"] = r(n), r(STEPS, n)
    for k, n in enumerate(N_MULTI):
        inp[f"c4/p{k}"], inp[f"c4/g{k}"] = r(n), r(STEPS, n)
    for k, n in enumerate(N_CLIP):
        inp[f"c6/p{k}"] = r(n)
        if k > 0:
            inp[f"c6/g{k}"] = r(STEPS, n)
    inp["c6/g2"][1, 5] = float("nan")       # step 2 only
    return inp


class _Group:
    def __init__(self, p, mirror=True):
        n = p.numel()
        self.p = p.cuda().clone()
        self.m = torch.zeros(n, device="cuda")
        self.v = torch.zeros(n, device="cuda")
        self.st = torch.zeros(3, device="cuda")
        self.mir = (torch.zeros(n, device="cuda", dtype=torch.bfloat16)
                    if mirror else None)
        self.g = torch.full((n,), -9.0, device="cuda")

    def items(self, tag):
        for k in ("p", "m", "v", "st", "g", "mir"):
            if getattr(self, k) is not None:
                yield f"{tag}{k}", getattr(self, k)


def _multi_args(groups):
    return ([g.p for g in groups], [g.g for g in groups],
            [g.m for g in groups], [g.v for g in groups],
            [g.st for g in groups], [LR] * len(groups), B1, B2, EPS,
            [g.mir if g.mir is not None else torch.Tensor() for g in groups])


def _arena(inp, step):
    """A different row order (and spare row) every step, from one array."""
    return inp["arena"].roll(step, 0).cuda().contiguous()


def run_cases(ext, inp):
    """Replay every case; returns {name: cpu tensor} of all that was written."""
    out = {}

    def rec(case, step, pairs):
        torch.cuda.synchronize()
        for k, t in pairs:
            out[f"{case}/{k}/{step}"] = t.detach().cpu().clone()

    # 1. adam_step_: step size from the host
    a = _Group(inp["c1/p"], mirror=False)
    for s in range(STEPS):
        a.g.copy_(inp["c1/g"][s])
        ext.adam_step_(a.p, a.g, a.m, a.v, s + 1, LR, B1, B2, EPS)
        rec("c1", s, [(k, t) for k, t in a.items("") if k != "st"])

    # 2. adam_step_dev_: own prolog, mirror
    for n in N_DEV:
        a = _Group(inp[f"c2_{n}/p"])
        for s in range(STEPS):
            a.g.copy_(inp[f"c2_{n}/g"][s])
            ext.adam_step_dev_(a.p, a.g, a.m, a.v, a.st, LR, B1, B2, EPS,
                               a.mir, 0)
            rec(f"c2_{n}", s, a.items(""))

    # 3. adam_prolog_many (4 states, rng) + adam_step_dev_ on the arena
    a = _Group(inp["c3/p"])
    states = [a.st] + [torch.zeros(3, device="cuda") for _ in range(3)]
    rng = torch.tensor([41], dtype=torch.int64, device="cuda")
    for s in range(STEPS):
        ext.adam_prolog_many(states, list(LRS4), B1, B2, rng)
        ext.adam_step_dev_(a.p, a.g, a.m, a.v, a.st, LRS4[0], B1, B2, EPS,
                           a.mir, 1, _arena(inp, s), S)
        rec("c3", s, list(a.items("")) + [("rng", rng)]
            + [(f"st{k}", t) for k, t in enumerate(states)])

    # 4. adam_step_multi_: 3 groups, own prolog, rng bump, mirrors on 0 and 2
    gs = [_Group(inp[f"c4/p{k}"], mirror=k != 1) for k in range(3)]
    rng = torch.tensor([7], dtype=torch.int64, device="cuda")
    for s in range(STEPS):
        for k, g in enumerate(gs):
            g.g.copy_(inp[f"c4/g{k}"][s])
        ext.adam_step_multi_(*_multi_args(gs), rng, 0)
        rec("c4", s, [kv for k, g in enumerate(gs) for kv in g.items(f"{k}")]
            + [("rng", rng)])

    # 5. adam_step_multi_: arena on group 0, trailing Polyak range + mirror
    gs = [_Group(inp["c5/p0"]), _Group(inp["c5/p1"], mirror=False)]
    tgt = inp["tgt"].cuda().clone()
    tmir = torch.zeros(NP, device="cuda", dtype=torch.bfloat16)
    for s in range(STEPS):
        gs[1].g.copy_(inp["c5/g1"][s])
        ext.adam_step_multi_(*_multi_args(gs), None, 0, _arena(inp, s), S,
                             tgt, inp["src"][s].cuda(), TAU, tmir)
        rec("c5", s, [kv for k, g in enumerate(gs) for kv in g.items(f"{k}")]
            + [("tgt", tgt), ("tmir", tmir)])

    # 6. adam_step_clip_: arena on group 0 (clipped), group 1 under its
    # threshold, group 2 guarded only with a NaN on step 2; shared counter
    gs = [_Group(inp[f"c6/p{k}"], mirror=k < 2) for k in range(3)]
    tgt = inp["tgt"].cuda().clone()
    tmir = torch.zeros(NP, device="cuda", dtype=torch.bfloat16)
    slots = torch.zeros(3 * 256, device="cuda")
    cs = [torch.zeros(3, device="cuda") for _ in range(3)]
    skips = torch.zeros(1, dtype=torch.int32, device="cuda")
    for s in range(STEPS):
        for k in (1, 2):
            gs[k].g.copy_(inp[f"c6/g{k}"][s])
        ext.adam_step_clip_(*_multi_args(gs), slots, list(CLIP_MAX), cs,
                            [skips] * 3, None, 0, _arena(inp, s), S,
                            tgt, inp["src"][s].cuda(), TAU, tmir)
        rec("c6", s, [kv for k, g in enumerate(gs) for kv in g.items(f"{k}")]
            + [("tgt", tgt), ("tmir", tmir), ("slots", slots),
               ("skips", skips)]
            + [(f"cs{k}", t) for k, t in enumerate(cs)])

    # 7. polyak_ alone, with a mirror
    for tag, tau in (("c7_tau", TAU), ("c7_one", 1.0)):
        tgt = inp["tgt"].cuda().clone()
        tmir = torch.zeros(NP, device="cuda", dtype=torch.bfloat16)
        for s in range(STEPS):
            ext.polyak_(tgt, inp["src"][s].cuda(), tau, tmir)
            rec(tag, s, [("tgt", tgt), ("tmir", tmir)])
    return out


def to_numpy(t):
    """bf16 has no numpy dtype: stored as its int16 bits."""
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy()


def main():
    from distributed_sac_amd.ops import native
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    inp = make_inputs()
    out = run_cases(native(), inp)
    again = run_cases(native(), inp)
    assert all(torch.equal(bits(out[k]), bits(again[k]))
               for k in out), "the kernels are not deterministic"
    arrays = {f"in/{k}": to_numpy(v) for k, v in inp.items()}
    arrays.update({f"out/{k}": to_numpy(v) for k, v in out.items()})
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(inp)} inputs, {len(out)} outputs, "
          f"{os.path.getsize(path)} bytes")


def bits(t):
    """Bit view for comparison: NaN equals itself, -0 differs from +0."""
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


if __name__ == "__main__":
    main()
