"""The update-path resolver and the opt-in modes' support rules
(distributed_sac_amd/algo/support.py), asked directly with hand-built
facts: every rule of every mode, GPU-only ones included, on the CPU.  The
expected paths and messages are literals; the engines that gather the facts
are covered by the modes' own tests."""

import itertools

import pytest

from distributed_sac_amd.algo.support import RULES, unsupported, update_path

# (on_gpu, precision, native, no_manual, manual_ok) -> path
PATHS = {
    (False, "fp32", False, False, False): "torch",
    (False, "fp32", False, False, True): "torch",
    (False, "fp32", False, True, False): "torch",
    (False, "fp32", False, True, True): "torch",
    (False, "fp32", True, False, False): "torch",
    (False, "fp32", True, False, True): "torch",
    (False, "fp32", True, True, False): "torch",
    (False, "fp32", True, True, True): "torch",
    (False, "bf16", False, False, False): "torch",
    (False, "bf16", False, False, True): "torch",
    (False, "bf16", False, True, False): "torch",
    (False, "bf16", False, True, True): "torch",
    (False, "bf16", True, False, False): "torch",
    (False, "bf16", True, False, True): "torch",
    (False, "bf16", True, True, False): "torch",
    (False, "bf16", True, True, True): "torch",
    (True, "fp32", False, False, False): "torch",
    (True, "fp32", False, False, True): "torch",
    (True, "fp32", False, True, False): "torch",
    (True, "fp32", False, True, True): "torch",
    (True, "fp32", True, False, False): "fp32",
    (True, "fp32", True, False, True): "fp32",
    (True, "fp32", True, True, False): "fp32",
    (True, "fp32", True, True, True): "fp32",
    (True, "bf16", False, False, False): "torch",
    (True, "bf16", False, False, True): "torch",
    (True, "bf16", False, True, False): "torch",
    (True, "bf16", False, True, True): "torch",
    (True, "bf16", True, False, False): "bf16-autograd",
    (True, "bf16", True, False, True): "bf16-manual",
    (True, "bf16", True, True, False): "bf16-autograd",
    (True, "bf16", True, True, True): "bf16-autograd",
}


def test_path_table_is_the_full_cross_product():
    assert set(PATHS) == set(itertools.product(
        (False, True), ("fp32", "bf16"), (False, True), (False, True),
        (False, True)))


@pytest.mark.parametrize("facts,path", PATHS.items(),
                         ids=lambda v: v if isinstance(v, str) else None)
def test_update_path(facts, path):
    assert update_path(*facts) == path
    if facts[4]:    # SACEngine: no manual preconditions, the default
        assert update_path(*facts[:4]) == path


PER, TQC, LN, PCGRAD = ("prioritized replay", "truncated quantile critics",
                        "critic_layer_norm", "pcgrad")
PER_GPU = ("prioritized replay: on a GPU only the bf16 manual-backward path "
           "carries importance-sampling weights (not the fp32 fused path)")
TQC_GPU = ("truncated quantile critics: on a GPU only the bf16 "
           "manual-backward path has the quantile loss kernels (not the "
           "fp32 path, not DSAC_NO_MANUAL=1)")


def facts(**over):
    f = dict(variant="mtsac", ddp=False, ref_weighting=False, path="torch",
             T=3, B=None, per=False, pcgrad=False, krng=True)
    assert set(over) <= set(f)
    f.update(over)
    return f


# one case per rule, in the rules' order (test_every_rule_has_its_case)
REFUSED = [
    (PER, dict(variant="care"),
     "prioritized replay: CAREEngine has no prioritized-replay path"),
    (PER, dict(ddp=True),
     "prioritized replay: not supported with a data-parallel group "
     "attached"),
    (PER, dict(ref_weighting=True),
     "prioritized replay: not defined for weighted_loss_mode='reference'"),
    (PER, dict(path="fp32"), PER_GPU),
    (TQC, dict(variant="care"),
     "truncated quantile critics: CAREEngine has no quantile-critic path"),
    (TQC, dict(per=True),
     "truncated quantile critics: not supported together with prioritized "
     "replay"),
    (TQC, dict(ref_weighting=True),
     "truncated quantile critics: not defined for "
     "weighted_loss_mode='reference'"),
    (TQC, dict(path="fp32"), TQC_GPU),
    (LN, dict(variant="care"),
     "critic_layer_norm: CAREEngine has no LayerNorm critic path"),
    (LN, dict(path="fp32"),
     "critic_layer_norm: on a GPU only the bf16 manual-backward path has "
     "the LN chain kernels (not the fp32 GPU path)"),
    (LN, dict(path="bf16-autograd"),
     "critic_layer_norm: the autograd bf16 path (DSAC_NO_MANUAL=1) has no "
     "LN chain kernels"),
    (LN, dict(path="bf16-manual", pcgrad=True, B=24),
     "critic_layer_norm: with pcgrad on a GPU each task's share of the "
     "batch (24 / 3 rows) must be a multiple of the chain kernels' 16-row "
     "tile"),
    (PCGRAD, dict(variant="care"),
     "pcgrad: CAREEngine has no per-task gradient arena"),
    (PCGRAD, dict(T=17),
     "pcgrad: num_tasks must be in 2..16 (variant mtsac), got 17"),
    (PCGRAD, dict(ddp=True),
     "pcgrad: not supported with a data-parallel group attached (the "
     "[T, numel] arena would need the all-reduce)"),
    (PCGRAD, dict(ref_weighting=True),
     "pcgrad: not defined for weighted_loss_mode='reference'"),
    (PCGRAD, dict(path="fp32"),
     "pcgrad: on a GPU only the bf16 manual-backward path writes per-task "
     "gradients (not the fp32 GPU path)"),
    (PCGRAD, dict(path="bf16-autograd"),
     "pcgrad: the autograd bf16 path (DSAC_NO_MANUAL=1) has no arena"),
    (PCGRAD, dict(path="bf16-manual", krng=False),
     "pcgrad: the visiting orders come from the device counter RNG "
     "(DSAC_KRNG=0 turns it off)"),
    (PCGRAD, dict(B=16),
     "pcgrad: the batch (16 rows) must divide into num_tasks = 3 equal "
     "parts (B % T != 0)"),
]

# the other side of a rule that covers two paths or two ends of a range,
# and for each mode two rules true at once: the earlier one wins
REFUSED_MORE = [
    (PER, dict(path="bf16-autograd"), PER_GPU),
    (TQC, dict(path="bf16-autograd"), TQC_GPU),
    (PCGRAD, dict(T=1),
     "pcgrad: num_tasks must be in 2..16 (variant mtsac), got 1"),
    (PCGRAD, dict(path="bf16-manual", B=16),
     "pcgrad: the batch (16 rows) must divide into num_tasks = 3 equal "
     "parts (B % T != 0)"),
    (PER, dict(ddp=True, path="fp32"), REFUSED[1][2]),
    (TQC, dict(per=True, ref_weighting=True), REFUSED[5][2]),
    (LN, dict(variant="care", path="fp32"), REFUSED[8][2]),
    (LN, dict(path="bf16-autograd", pcgrad=True, B=24), REFUSED[10][2]),
    (PCGRAD, dict(T=17, ddp=True), REFUSED[13][2]),
    (PCGRAD, dict(path="fp32", krng=False, B=16), REFUSED[16][2]),
]


@pytest.mark.parametrize("mode,over,message", REFUSED + REFUSED_MORE)
def test_refused(mode, over, message):
    assert unsupported(mode, facts(**over)) == message


def test_every_rule_has_its_case():
    """REFUSED walks the rule lists in order: the message of case i (which
    test_refused asserts) is the one of rule i."""
    assert [m for m, _, _ in REFUSED] == \
        [m for m, rules in RULES.items() for _ in rules]
    whys = [why for rules in RULES.values() for _, why in rules]
    for (mode, over, message), why in zip(REFUSED, whys):
        assert message == f"{mode}: " + why.format(max_T=16, **facts(**over))


@pytest.mark.parametrize("mode,over", [
    (PER, dict()), (PER, dict(path="bf16-manual")),
    (TQC, dict()), (TQC, dict(path="bf16-manual")),
    (LN, dict()), (LN, dict(path="bf16-manual")),
    # the 16-row tile binds PCGrad's task shares on the GPU only
    (LN, dict(pcgrad=True, B=24)),
    (LN, dict(path="bf16-manual", pcgrad=True, B=48)),
    (LN, dict(path="bf16-manual", B=24)),
    (PCGRAD, dict()), (PCGRAD, dict(path="bf16-manual")),
    (PCGRAD, dict(T=2, B=16)), (PCGRAD, dict(T=16, B=16)),
    (PCGRAD, dict(path="bf16-manual", B=48)),
    # the torch path draws its visiting orders on the host
    (PCGRAD, dict(krng=False)),
    # a mode's rules do not look at the other modes' facts
    (PER, dict(pcgrad=True, B=16)), (PCGRAD, dict(per=True)),
])
def test_supported(mode, over):
    assert unsupported(mode, facts(**over)) is None
