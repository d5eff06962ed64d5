"""Truncated quantile critics off the GPU: cfg validation, the CPU update,
checkpoints at a quantile head width and the unsupported combinations."""

import pytest
import torch

from distributed_sac_amd.algo import SACEngine, create_engine
from distributed_sac_amd.config import SACConfig, load_variant
from tests.test_engine import make_batch, small_cfg


def tqc_cfg(variant, M=5, drop=1):
    cfg = small_cfg(variant)
    cfg.critic_quantiles, cfg.critic_quantiles_drop = M, drop
    return cfg


@pytest.mark.parametrize("M,drop", [(33, 2), (5, -1), (5, 5), (2, None),
                                    (2.5, 0), (-1, 0)])
def test_cfg_rejects(M, drop):
    d = {"critic_quantiles": M}
    if drop is not None:
        d["critic_quantiles_drop"] = drop
    with pytest.raises(ValueError, match="critic_quantiles"):
        SACConfig.from_dict(d)


def test_cfg_precedence(monkeypatch):
    assert SACConfig().critic_quantiles_choice == (0, 2)
    monkeypatch.setenv("DSAC_CRITIC_QUANTILES", "25")
    assert SACConfig().critic_quantiles_choice == (25, 2)
    monkeypatch.setenv("DSAC_CRITIC_QUANTILES_DROP", "3")
    assert SACConfig().critic_quantiles_choice == (25, 3)
    cfg = SACConfig.from_dict({"critic_quantiles": 5})
    assert cfg.critic_quantiles_choice == (5, 3)     # the cfg's key wins
    assert SACConfig.from_dict(
        {"critic_quantiles": 0}).critic_quantiles_choice[0] == 0
    monkeypatch.setenv("DSAC_CRITIC_QUANTILES", "x")
    with pytest.raises(ValueError, match="DSAC_CRITIC_QUANTILES"):
        SACConfig().critic_quantiles_choice


@pytest.mark.parametrize("variant", ["sac", "mtsac"])
def test_cpu_update_and_checkpoint(variant):
    torch.manual_seed(0)
    cfg = tqc_cfg(variant)
    e = SACEngine(cfg, "cpu")
    before = [g.flat_data.clone() for g in
              (e.critic_group, e.actor_group, e.alpha_group)]
    m = e.update(make_batch(cfg))
    assert all(v == v for v in m.values())
    for b, g in zip(before, (e.critic_group, e.actor_group, e.alpha_group)):
        assert not torch.equal(b, g.flat_data)

    # round trip at head width 5: same keys as a scalar engine, same update
    ckpt = e.checkpoint_state()
    scalar = SACEngine(small_cfg(variant), "cpu")
    name = "local_critic_1" if variant == "sac" else "local_critic"
    assert ckpt[name].keys() == scalar.checkpoint_state()[name].keys()
    e2 = SACEngine(cfg, "cpu")
    e2.load_checkpoint_state(ckpt)
    eps = [torch.randn(cfg.batch_size, cfg.action_dim) for _ in range(2)]
    e._eps_queue = [x.clone() for x in eps]
    e2._eps_queue = [x.clone() for x in eps]
    assert e.update(make_batch(cfg, seed=1)) == \
        e2.update(make_batch(cfg, seed=1))

    # scalar <-> quantile: an error that names both widths
    with pytest.raises(ValueError, match="width 5.* has 1"):
        scalar.load_checkpoint_state(ckpt)
    with pytest.raises(ValueError, match="width 1.* has 5"):
        e2.load_checkpoint_state(scalar.checkpoint_state())


def test_unsupported_combinations():
    care = load_variant("care")
    care.critic_quantiles = 5
    with pytest.raises(NotImplementedError, match="CAREEngine"):
        create_engine(care, "cpu")
    cfg = tqc_cfg("mtsac")
    cfg.weighted_loss_mode = "reference"
    with pytest.raises(NotImplementedError, match="reference"):
        SACEngine(cfg, "cpu")
    e = SACEngine(tqc_cfg("mtsac"), "cpu")
    batch = make_batch(e.cfg)
    batch["is_weights"] = torch.ones(e.cfg.batch_size)
    batch["indices"] = torch.zeros(e.cfg.batch_size, 2, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="prioritized"):
        e.update_tensors(batch)
