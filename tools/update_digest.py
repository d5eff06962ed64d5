"""Bit-exact digest of the bf16 manual update, for before/after
comparison of a change that must not alter results.

For each engine config x DSAC_FUSE_TAIL in {1, 0}: 6 update_tensors
calls (counter RNG on) over three fixed batches, then the SHA-256 of
every flat parameter group and of the six metric dicts.  Then the same
with prioritized batches, with a forced world-1 data-parallel group
attached, and with that group through capture_dp / dp_graphed_update.  Uses the
engines' public API only, so the same file runs on any commit:

    python tools/update_digest.py > digest.txt     # on both commits
"""

import hashlib
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from distributed_sac_amd.algo import CAREEngine, SACEngine  # noqa: E402
from distributed_sac_amd.config import load_variant  # noqa: E402
from tests.test_care import care_cfg  # noqa: E402
from tests.test_engine import make_batch, small_cfg  # noqa: E402


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(
        t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()


def fill_replay(cfg):
    from distributed_sac_amd.replay import ShardedReplay
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
    return replay


def run(name, make_cfg, engine_cls, fuse, per=False, ddp=None, graphs=False):
    """per: the batches carry IS weights and indices (no replay attached).
    ddp: a data-parallel group to attach.  graphs: capture_dp, then
    dp_graphed_update instead of update_tensors."""
    os.environ["DSAC_FUSE_TAIL"] = fuse
    torch.manual_seed(0)
    cfg = make_cfg()
    e = engine_cls(cfg, "cuda:0", precision="bf16")
    if ddp is not None:
        e.attach_ddp(ddp)
    B = cfg.batch_size
    batches = [{k: v.cuda() for k, v in make_batch(cfg, B, seed=s).items()}
               for s in range(3)]
    if per:
        g = torch.Generator().manual_seed(11)
        for b in batches:
            b["is_weights"] = (1.0 - torch.rand(B, generator=g)).cuda()
            b["indices"] = torch.arange(B, device="cuda")
    tag = f"{name} fuse_tail={fuse}"
    if graphs:
        e.capture_dp(fill_replay(cfg), B)
    metrics = []
    for i in range(6):
        try:
            m = (e.dp_graphed_update() if graphs else e.update_tensors(
                {k: v.clone() for k, v in batches[i % 3].items()}))
        except NotImplementedError:
            # prioritized batches need the fused tail
            print(f"{tag} raises NotImplementedError")
            return
        metrics.append(torch.stack([m[k].float().reshape(())
                                    for k in sorted(m)]).clone())
    torch.cuda.synchronize()
    for g in ("alpha", "actor", "critic", "target", "context"):
        grp = getattr(e, g + "_group", None)
        if grp is not None:
            print(f"{tag} {g:8s} {sha(grp.flat_data)}")
    if per:
        print(f"{tag} newprio  {sha(e.per_new_priorities)}")
    print(f"{tag} metrics  {sha(torch.stack(metrics))}")
    assert all(torch.isfinite(x).all() for x in metrics), tag


def main():
    import torch.distributed as dist
    from distributed_sac_amd.parallel import DataParallelGroup
    tmp = tempfile.mkdtemp()
    cases = [
        ("sac_small", lambda: small_cfg("sac"), SACEngine),
        ("mtsac_small", lambda: small_cfg("mtsac"), SACEngine),
        ("mtsac_shipped", lambda: load_variant("mtsac"), SACEngine),
        ("care_modified", lambda: care_cfg(tmp, modified=True), CAREEngine),
        ("care_original",
         lambda: care_cfg(tmp, modified=False, num_tasks=1), CAREEngine),
    ]
    for name, make_cfg, cls in cases:
        for fuse in ("1", "0"):
            run(name, make_cfg, cls, fuse)
    for fuse in ("1", "0"):
        run("mtsac_small+per", cases[1][1], SACEngine, fuse, per=True)
    # a forced world-1 group: the `ddp is not None` fold branches, eagerly
    # and through the three segment graphs
    ddp = DataParallelGroup(device=torch.device("cuda:0"), force=True)
    try:
        for graphs in (False, True):
            for name, make_cfg, cls in (cases[1], cases[3], cases[4]):
                for fuse in ("1", "0"):
                    run(name + ("+dp_graphs" if graphs else "+dp"),
                        make_cfg, cls, fuse, ddp=ddp, graphs=graphs)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
