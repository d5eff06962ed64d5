"""Host-side driver of the MLP-chain kernels for the manual bf16 update.

One :class:`ManualChain` per MLP chain (critic twin, target twin, actor
head, original-CARE context encoder) owns what the chain kernels need
besides the bf16 weight mirror: the fragment-packed weight buffers, the
W^T shape carriers of the dx kernel and the chain's word offsets into its
flat gradient.  ``forward`` / ``input_grad`` / ``backward`` hide the two
kernel modes: the fused chain kernels (default) and the per-layer kernels
(``DSAC_CHAIN=0``).  Both issue the same math; the per-layer mode needs no
packed weights.
"""

from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import torch

from . import native
from .flat import FlatParams


def use_chain() -> bool:
    """Fused MLP-chain kernels (one launch per chain, in-kernel f32
    concat+cast input).  DSAC_CHAIN=0 restores the per-layer path."""
    return os.environ.get("DSAC_CHAIN", "1") == "1"


def frag_numel(rows: int, cols: int, G: int = 1) -> int:
    """bf16 elements of a fragment-packed [G, rows, cols] operand
    (k_bf16_pack_frag: 16x32 tiles of 512 elements).  The forward pack of
    a [N, K] weight is (N, K); the dx pack is its transpose, (K, N)."""
    return G * ((rows + 15) // 16) * ((cols + 31) // 32) * 512


def mlp_bwd_arena(ext, dy, acts, wsh, w_offs, b_offs, arena, S, chunk,
                  G=1, transpose_w=0):
    """Per-layer backward of an act-fwd chain; dW/db partials go to the
    phase arena at the layers' flat-grad offsets (fold happens once per
    phase).  Returns dy at the first layer's output."""
    n = len(wsh)
    for i in range(n - 1, -1, -1):
        act = 1 if i < n - 1 else 0
        yout = acts[i + 1] if i < n - 1 else acts[i]
        ext.linear_bwd_dwdb_arena(dy, acts[i], yout, act, G, arena,
                                  w_offs[i], b_offs[i], S, chunk,
                                  transpose_w)
        if i > 0:
            dy = ext.linear_bwd_dx_bf16(dy, wsh[i], yout, act, G, 0)
    return dy


class ManualChain:
    """One ReLU MLP chain (linear last layer) of the manual update.

    ws16: bf16 weight views into the flat mirror, [G,N,K] ([N,K] for G=1);
    bs: the fp32 biases.  ``group`` with ``w_params`` / ``b_params`` (the
    parameters whose .grad receives dW/db; for a twin stack the Q1 half,
    Q2 follows it) fixes the flat-gradient offsets; a chain that is never
    differentiated passes none.  ``dx=False`` skips the dx-side buffers
    (target twin).  ``always_chain`` pins the chain kernels regardless of
    DSAC_CHAIN (context encoder)."""

    def __init__(self, ws16: Sequence[torch.Tensor],
                 bs: Sequence[torch.Tensor], G: int = 1,
                 group: Optional[FlatParams] = None,
                 w_params: Sequence[torch.Tensor] = (),
                 b_params: Sequence[torch.Tensor] = (),
                 dx: bool = True, always_chain: bool = False):
        self.ws16 = list(ws16)
        self.bs = list(bs)
        self.G = int(G)
        self._always_chain = always_chain
        dev = self.ws16[0].device

        def buf(*shape):
            return torch.empty(*shape, dtype=torch.bfloat16, device=dev)

        nk = [(w.numel() // (G * w.shape[-1]), w.shape[-1])
              for w in self.ws16]
        # FRAGMENT-PACKED weight mirrors: the chain kernels' B-operand
        # loads become base + lane*16 unit-stride; re-packed per update by
        # pack_chains
        self.fwd_frag = [buf(frag_numel(N, K, G)) for N, K in nk]
        self.dx_frag = [buf(frag_numel(K, N, G)) for N, K in nk] if dx \
            else None
        # W^T shape carriers for the dx binding (values come from dx_frag)
        self._wt = [buf(G, K, N) if G > 1 else buf(K, N)
                    for N, K in nk] if dx else None
        self._empty = buf(0)
        self._aflags = [1] * (len(nk) - 1) + [0]

        def offs(ps):
            return [group.offsets[next(j for j, q in enumerate(group.params)
                                       if q is p)] for p in ps]
        self.w_offs: List[int] = offs(w_params)
        self.b_offs: List[int] = offs(b_params)

    @property
    def chain_mode(self) -> bool:
        return self._always_chain or use_chain()

    def _youts(self, acts):
        return list(acts[1:len(self.ws16)]) + [self._empty]

    def _fwd_args(self, x1, x2=None, *, rowcat=False, save_acts=True,
                  out_f32=True, act_last=0):
        """forward()'s arguments as one job of the pair binding."""
        return (x1, x2 if x2 is not None else x1.new_empty(0),
                self.ws16, [b.contiguous() for b in self.bs],
                int(act_last), self.G, 1 if out_f32 else 0,
                1 if rowcat else 0, 1 if save_acts else 0, self.fwd_frag)

    @torch.no_grad()
    def forward(self, x1, x2=None, *, rowcat=False, save_acts=True,
                out_f32=True, act_last=0):
        """y = chain([x1 | x2]) (``rowcat``: x1 over x2 by rows).  Returns
        (y, acts): y is [M,N] or [G,M,N]; acts = [bf16 input, hidden
        activations...], what input_grad/backward consume."""
        ext = native()
        if self.chain_mode:
            out = ext.mlp_chain_fwd_bf16(
                x1, x2 if x2 is not None else x1.new_empty(0),
                self.ws16, [b.contiguous() for b in self.bs],
                int(act_last), self.G, 1 if out_f32 else 0, 0,
                1 if rowcat else 0, 1 if save_acts else 0, self.fwd_frag)
            return out[0], [out[1]] + list(out[2:])
        if x2 is not None:
            if x1.dtype != x2.dtype:
                x1, x2 = x1.to(torch.bfloat16), x2.to(torch.bfloat16)
            x1 = torch.cat([x1, x2], dim=0 if rowcat else -1)
        h = x1.to(torch.bfloat16)
        acts = [h]
        n = len(self.ws16)
        for i in range(n):
            last = i == n - 1
            h = ext.linear_act_fwd_bf16(
                h, self.ws16[i], self.bs[i].contiguous(),
                int(act_last) if last else 1, self.G,
                (1 if out_f32 else 0) if last else 0)
            if not last:
                acts.append(h)
        return h, acts

    @torch.no_grad()
    def input_grad(self, dy, acts, lo):
        """dx-only walk (no dW/db): fp32 gradient w.r.t. input columns
        ``lo:``, per group [G,M,K0-lo] — the per-layer mode returns the
        groups already summed, [M,K0-lo]."""
        ext = native()
        if self.chain_mode:
            return ext.mlp_chain_dx_bf16(
                dy, self._wt, self._youts(acts), acts[0].shape[-1],
                self._aflags, self.G, 0, int(lo), self.dx_frag)[-1]
        n = len(self.ws16)
        for i in range(n - 1, 0, -1):
            dy = ext.linear_bwd_dx_bf16(
                dy, self.ws16[i], acts[i + 1] if i < n - 1 else acts[i],
                self._aflags[i], self.G, 0)
        return self._dx0_per_layer(ext, dy, acts)[:, lo:].float()

    def _dx0_per_layer(self, ext, dy, acts):
        n = len(self.ws16)
        return ext.linear_bwd_dx_bf16(
            dy, self.ws16[0], acts[1] if n > 1 else acts[0],
            1 if n > 1 else 0, self.G, 1)

    @torch.no_grad()
    def backward(self, dy, acts, arena, S, chunk, *, rows=None, dx0_lo=-1):
        """Full backward: dW/db split-K partials into ``arena`` at the
        chain's flat-grad offsets.  ``rows`` selects a row range of
        batched activations.  With ``dx0_lo >= 0`` returns the bf16
        gradient w.r.t. input columns ``dx0_lo:``, summed over groups."""
        ext = native()
        n = len(self.ws16)
        if rows is not None:
            acts = [a[..., rows, :] for a in acts]
        if not self.chain_mode:
            dy = mlp_bwd_arena(ext, dy, acts, self.ws16, self.w_offs,
                               self.b_offs, arena, S, chunk, self.G)
            if dx0_lo < 0:
                return None
            return self._dx0_per_layer(ext, dy, acts)[:, dx0_lo:]
        outs = ext.mlp_chain_dx_bf16(
            dy, self._wt, self._youts(acts), acts[0].shape[-1],
            self._aflags, self.G, 1, int(dx0_lo), self.dx_frag)
        dx0 = None
        if dx0_lo >= 0:
            dx0 = outs[n][0]
            for g in range(1, self.G):
                dx0 = dx0 + outs[n][g]
            dx0 = dx0.to(torch.bfloat16)
        ext.dwdb_grouped_arena(list(outs[:n]), list(acts[:n]), arena,
                               self.w_offs, self.b_offs, self.G, S, chunk)
        return dx0


def use_pair_fwd() -> bool:
    """Two independent forward chains in one launch (forward_pair).
    DSAC_PAIR_FWD=0 restores the two separate launches."""
    return os.environ.get("DSAC_PAIR_FWD", "1") != "0"


@torch.no_grad()
def forward_pair(a, b):
    """``chain.forward(*args, **kwargs)`` of two INDEPENDENT chains, each
    given as ``(chain, args, kwargs)``; returns the two results.  With both
    chains on the chain kernels this is one k_bf16_chain_fwd_pair launch
    (same bits; a ``save_acts=False`` job's acts[0] comes back empty),
    otherwise the two forward calls in the given order.  DSAC_PAIR_RM=2
    selects 32-row tiles (measurement only)."""
    (ca, args_a, kw_a), (cb, args_b, kw_b) = a, b
    if not (ca.chain_mode and cb.chain_mode and use_pair_fwd()):
        return ca.forward(*args_a, **kw_a), cb.forward(*args_b, **kw_b)
    rm = 2 if os.environ.get("DSAC_PAIR_RM", "1") == "2" else 1
    outs = native().mlp_chain_fwd_pair_bf16(
        *ca._fwd_args(*args_a, **kw_a), *cb._fwd_args(*args_b, **kw_b), rm)
    return tuple((o[0], [o[1]] + list(o[2:])) for o in outs)


def pack_chains(ext, entries: Sequence[Tuple[ManualChain, bool, bool]]):
    """ONE pack_weights_frag launch re-packs the listed chains' weight
    mirrors into the fragment layout: per ``(chain, fwd, dx)`` the forward
    and/or dx set.  Chains in per-layer mode need no pack and are skipped.
    """
    ws, ps, gs, dxs = [], [], [], []
    for chain, fwd, dx in entries:
        if not chain.chain_mode:
            continue
        for flag, frags in ((0, chain.fwd_frag if fwd else None),
                            (1, chain.dx_frag if dx else None)):
            if frags is not None:
                ws += chain.ws16
                ps += frags
                gs += [chain.G] * len(frags)
                dxs += [flag] * len(frags)
    if ws:
        ext.pack_weights_frag(ws, ps, gs, dxs)
