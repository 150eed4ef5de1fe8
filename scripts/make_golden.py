#!/usr/bin/env python
"""Record what the reference implementation computes for the differential host tests.

``python scripts/make_golden.py --reference DIR`` imports the reference's ``model``,
``memory`` and ``utils`` modules from DIR (tests/refimport.py), drives them through the
same seeded scripts the tests run on this framework's classes (the ``_drive_*`` / ``_ref_*``
/ ``record_*`` functions of the test modules) and stores inputs, weights and results as
``tests/golden/*.npz``.  The tests read only those files.  Re-run it when a test's script
changes; the recorded arrays hold data only, no reference code.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference implementation")
    a = ap.parse_args()

    from tests import goldens, refimport
    from tests import test_aql_reference_host as t_aql
    from tests import test_models_host as t_models
    from tests import test_nstep_host as t_nstep
    from tests import test_replay_host as t_replay
    from tests import test_trainers_host as t_trainers

    refimport.configure(a.reference)
    if not refimport.available():
        raise SystemExit(f"no reference checkout at {a.reference}")
    ref_model, ref_memory, ref_utils = (refimport.load(n) for n in ("model", "memory", "utils"))
    written = []

    # replay / n-step (tests/test_replay_host.py, tests/test_nstep_host.py)
    written.append(goldens.save("replay_per", t_replay._drive_per(ref_memory.PrioritizedReplayBuffer(100, 0.6))))
    b = t_replay._drive_custom_per(ref_memory.CustomPrioritizedReplayBuffer(64, 0.6))
    written.append(goldens.save("replay_custom_per", {
        "obs": np.stack([np.asarray(x) for x in b[0]]), "obs_is_list": isinstance(b[0], list),
        "next_obs_is_list": isinstance(b[3], list), "weights": np.asarray(b[-2]),
        "idxes": np.asarray(b[-1], dtype=np.int64)}))
    written.append(goldens.save("nstep_reference_mode", t_nstep._drive_reference_mode(
        ref_memory.BatchStorage(3, 0.99), raises_on_lone_done=True)))

    # models (tests/test_models_host.py)
    env, ours, x = t_models._dueling_forward_case()
    theirs = ref_model.DuelingDQN(env)
    ref_sd = theirs.state_dict()   # the reference's own checkpoint layout, before anything is loaded
    rec = {"ref_keys": np.array(list(ref_sd), dtype=np.str_),
           "ref_dtypes": np.array([str(v.dtype) for v in ref_sd.values()], dtype=np.str_),
           "ref_shapes": np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in ref_sd.values()], dtype=np.int64)}
    theirs.load_state_dict(ours.state_dict())
    rec.update(t_models._dueling_outputs(theirs, x))
    written.append(goldens.save("models_dueling", rec))

    from apex_amd.envs import make

    for env_id in t_models.AQL_FORWARD_ENVS:
        env = make(env_id)
        torch.manual_seed(0)
        theirs = ref_model.AQL(env, propose_sample=2, uniform_sample=5, device="cpu")
        s = np.asarray(env.reset())
        rec = {"s": s}
        goldens.put_state(rec, "state", theirs.state_dict())
        rec.update(t_models._aql_act(theirs, s))
        written.append(goldens.save("models_aql_" + env_id, rec))

    env, model, tgt, batch = t_models._loss_case()
    rec = {}
    goldens.put_state(rec, "model", model.state_dict())
    goldens.put_state(rec, "target", tgt.state_dict())
    rec.update(t_models._loss_and_update(ref_utils, model, tgt, batch))
    written.append(goldens.save("models_loss", rec))

    # checkpoint (tests/test_trainers_host.py)
    import tempfile

    from apex_amd.utils.checkpoint import save_model

    env, mine, x = t_trainers._checkpoint_case()
    with tempfile.TemporaryDirectory() as d:
        path = save_model(mine, os.path.join(d, "model0.pth"))
        sd = torch.load(path, map_location="cpu", weights_only=True)
    theirs = ref_model.DuelingDQN(env)
    theirs.load_state_dict(sd)
    rec = {"ref_forward": theirs.double()(x.double()).detach().numpy()}
    goldens.put_state(rec, "checkpoint", sd)
    written.append(goldens.save("trainers_checkpoint", rec))

    # AQL_dis learner steps (tests/test_aql_reference_host.py)
    for env_id in t_aql.AQL_DIS_ENVS:
        for k, rec in enumerate(t_aql.record_reference_steps(ref_model, ref_utils, env_id)):
            written.append(goldens.save(f"aql_dis_{env_id}_step{k}", rec))

    for p in written:
        print(f"{os.path.getsize(p):9d}  {os.path.relpath(p, ROOT)}")


if __name__ == "__main__":
    main()
