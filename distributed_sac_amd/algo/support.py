"""Which update path an engine runs and which opt-in modes that path
carries, as pure functions of plain facts: every combination can be asked
about on a CPU."""

from __future__ import annotations

from typing import Optional

from ..ops.torch_ref import PCGRAD_MAX_T


def update_path(on_gpu: bool, precision: str, native: bool,
                no_manual: bool, manual_ok: bool = True) -> str:
    """``torch`` (on the CPU, or the native kernels are not enabled and
    loadable: ``native``), ``fp32`` (the autograd GPU path),
    ``bf16-autograd`` (``no_manual``: DSAC_NO_MANUAL=1, or CARE without its
    manual preconditions ``manual_ok``) or ``bf16-manual`` (the
    three-segment hand-rolled backward)."""
    if not (on_gpu and native):
        return "torch"
    if precision != "bf16":
        return "fp32"
    return "bf16-manual" if manual_ok and not no_manual else "bf16-autograd"


_REF_WEIGHTING = ("ref_weighting",
                  "not defined for weighted_loss_mode='reference'")

# mode -> (condition of unsupported(), why) in order: the first condition that
# holds refuses the mode; ``why`` is formatted with the facts and PCGRAD_MAX_T
RULES = {
    "prioritized replay": [
        ("care", "CAREEngine has no prioritized-replay path"),
        ("ddp", "not supported with a data-parallel group attached"),
        _REF_WEIGHTING,
        ("autograd_gpu", "on a GPU only the bf16 manual-backward path carries "
         "importance-sampling weights (not the fp32 fused path)"),
    ],
    "truncated quantile critics": [
        ("care", "CAREEngine has no quantile-critic path"),
        ("per", "not supported together with prioritized replay"),
        _REF_WEIGHTING,
        ("autograd_gpu", "on a GPU only the bf16 manual-backward path has the "
         "quantile loss kernels (not the fp32 path, not "
         "DSAC_NO_MANUAL=1)"),
    ],
    "critic_layer_norm": [
        ("care", "CAREEngine has no LayerNorm critic path"),
        ("fp32", "on a GPU only the bf16 manual-backward path has the LN "
         "chain kernels (not the fp32 GPU path)"),
        ("bf16_autograd", "the autograd bf16 path (DSAC_NO_MANUAL=1) has no "
         "LN chain kernels"),
        ("pcgrad_tile", "with pcgrad on a GPU each task's share of the batch "
         "({B} / {T} rows) must be a multiple of "
         "the chain kernels' 16-row tile"),
    ],
    "pcgrad": [
        ("care", "CAREEngine has no per-task gradient arena"),
        ("bad_T", "num_tasks must be in 2..{max_T} (variant mtsac), got {T}"),
        ("ddp", "not supported with a data-parallel group attached (the "
         "[T, numel] arena would need the all-reduce)"),
        _REF_WEIGHTING,
        ("fp32", "on a GPU only the bf16 manual-backward path writes "
         "per-task gradients (not the fp32 GPU path)"),
        ("bf16_autograd",
         "the autograd bf16 path (DSAC_NO_MANUAL=1) has no arena"),
        ("no_krng", "the visiting orders come from the device counter RNG "
         "(DSAC_KRNG=0 turns it off)"),
        ("B % T", "the batch ({B} rows) must divide into num_tasks = {T} "
         "equal parts (B % T != 0)"),
    ],
}


def unsupported(mode: str, f: dict) -> Optional[str]:
    """Why ``mode`` does not run, or None if it does.  The facts ``f``:
    variant, ddp (an enabled data-parallel group is attached),
    ref_weighting (weighted_loss_mode='reference' is in effect), path, T
    (num_tasks), B (batch rows, None before the first batch), per (a
    prioritized replay is attached, or the batch carries is_weights),
    pcgrad, krng (DSAC_KRNG is on)."""
    path, T, B = f["path"], f["T"], f["B"]
    gpu = path != "torch"
    holds = {
        "care": f["variant"] == "care",
        "ddp": f["ddp"],
        "ref_weighting": f["ref_weighting"],
        "fp32": path == "fp32",
        "bf16_autograd": path == "bf16-autograd",
        "autograd_gpu": gpu and path != "bf16-manual",
        "per": f["per"],
        "bad_T": not 2 <= T <= PCGRAD_MAX_T,
        "no_krng": gpu and not f["krng"],
        "B % T": B is not None and B % T != 0,
        "pcgrad_tile": gpu and f["pcgrad"] and B is not None
        and (B // T) % 16 != 0,
    }
    for name, why in RULES[mode]:
        if holds[name]:
            return f"{mode}: " + why.format(max_T=PCGRAD_MAX_T, **f)
    return None
