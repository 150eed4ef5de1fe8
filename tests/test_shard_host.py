"""The n-step shard base (engine/shard.py): the ``st`` layout ``nstep_emit`` reads, written once."""
import torch

# key -> (shape, dtype) at E envs, A actions, n steps
E, A, N = 3, 5, 2
LAYOUT = {
    "win_ids": ((E, N, 4), torch.int32),
    "win_a": ((E, N), torch.int32),
    "win_r": ((E, N), torch.float32),
    "win_q": ((E, N, A), torch.float32),
    "win_meta": ((E, 4), torch.int32),
    "hist": ((E, 4), torch.int32),
    "drain_ids": ((E, N, 4), torch.int32),
    "drain_a": ((E, N), torch.int32),
    "drain_r": ((E, N), torch.float32),
    "drain_q": ((E, N), torch.float32),
    "drain_meta": ((E, 2), torch.int32),
    "drain_s2": ((E, 4), torch.int32),
}


def test_nstep_state_layout():
    from apex_amd.engine.shard import nstep_state

    st = nstep_state(E, A, N, "cpu")
    assert set(st) == set(LAYOUT) and len(st) == 12
    for k, (shape, dtype) in LAYOUT.items():
        assert tuple(st[k].shape) == shape, k
        assert st[k].dtype == dtype, k
        assert st[k].device.type == "cpu" and st[k].is_contiguous(), k
        assert not st[k].any(), k


def test_shards_share_the_base_and_the_action_key():
    from apex_amd.engine.actor_shard import ActorShard
    from apex_amd.engine.host_env import HostEnvShard
    from apex_amd.engine.shard import ACT_SEED_XOR, NStepShard
    from apex_amd.engine.vector import VectorActorShard

    for cls in (ActorShard, HostEnvShard, VectorActorShard):
        assert issubclass(cls, NStepShard), cls
    assert ACT_SEED_XOR == 0x5E1EC7
