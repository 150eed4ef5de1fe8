"""Hand-set policies in the MLP dueling net for the vector-engine rollout tests, and a host
model of one greedy episode (fp64 net, fp32 states, envs/classic.py).

A random-init net plays one constant action on both envs (CartPole episodes of 8 to 11 steps,
no MountainCar terminal at all), which exercises neither the argmax nor the row masking of
``vec_rollout``.  ``make_policy`` wires a linear controller through hidden units 0 and 1 of an
otherwise random, scaled-down net: the policy is "action A - 1 iff w . s > 0", with the random
remainder as live noise in every other unit."""
from __future__ import annotations

import numpy as np
import torch

from apex_amd import envs
from apex_amd.engine.vector import VECTOR_ENVS, make_model

# recipe -> (w per observation width, gain); seeds / noise levels the recipes were checked with
RECIPES = {
    "balance": ((0.01, 0.05, 1.0, 0.5), 10.0),   # CartPole: every episode runs to the time limit
    "angle": ((0.0, 0.0, 1.0, 0.0), 10.0),       # CartPole: every episode ends by a terminal, lengths differ
    "pump": ((0.0, 1.0), 100.0),                 # MountainCar: push along the velocity; reaches the goal
}
SEEDS = ((1, 0.02), (9, 0.02), (20, 0.1))        # (torch seed, noise scale)
R_STEP = {"CartPole-v0": 1.0, "CartPole-v1": 1.0, "MountainCar-v0": -1.0}
NEAR = 1e-4   # a next state this close to a termination threshold is not compared for its terminal flag


def make_policy(env_id: str, recipe: str, seed: int = 1, noise: float = 0.02):
    """fp32 CPU ``DuelingDQN`` of ``env_id`` holding ``recipe``."""
    w, gain = RECIPES[recipe]
    torch.manual_seed(seed)
    m = make_model(env_id)
    hi = m.num_actions - 1
    assert len(w) == m.input_shape[0], (env_id, recipe)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.2)
            p.mul_(noise)
        sd = dict(m.named_parameters())
        wt = torch.tensor(w, dtype=torch.float32) * gain
        sd["features.0.weight"][0] = wt
        sd["features.0.weight"][1] = -wt
        sd["features.0.bias"][:2] = 0
        wa = sd["advantage.0.weight"]
        wa[0] = 0
        wa[1] = 0
        wa[0, 0] = 1
        wa[1, 1] = 1
        sd["advantage.0.bias"][:2] = 0
        w2 = sd["advantage.2.weight"]
        w2[hi, 0] += 1
        w2[0, 1] += 1
        w2[0, 0] -= 1
        w2[hi, 1] -= 1
    return m


def load_policy(engine, model) -> None:
    """``model``'s weights into the engine's online net, in place (the flat buffer stays put)."""
    engine.learner.model.load_state_dict(model.state_dict())


def fp64(model):
    from apex_amd.models.dqn import DuelingDQN

    ref = DuelingDQN.from_shapes(tuple(model.input_shape), model.num_actions).double()
    ref.load_state_dict({k: v.detach().double().cpu() for k, v in model.state_dict().items()})
    return ref


def host_step(env, s, a):
    """envs/classic.py from fp32 state ``s`` (exact in fp64): (s' fp64, terminal, distance of
    s' from the nearest termination threshold)."""
    u = env.unwrapped
    u.state = tuple(float(v) for v in s)
    u.steps_beyond_done = None
    u.step(int(a))
    nxt = np.asarray(u.state, dtype=np.float64)
    if hasattr(u, "x_threshold"):
        term = bool(nxt[0] < -u.x_threshold or nxt[0] > u.x_threshold or nxt[2] < -u.theta_threshold_radians
                    or nxt[2] > u.theta_threshold_radians)
        margin = min(abs(abs(nxt[0]) - u.x_threshold), abs(abs(nxt[2]) - u.theta_threshold_radians))
    else:
        term = bool(nxt[0] >= u.goal_position)
        margin = abs(nxt[0] - u.goal_position)
    return nxt, term, float(margin)


def host_reset_draws(env_id: str, n: int, rng) -> np.ndarray:
    """Host-uniform reset states in the env's reset range, fp32 [n, obs]."""
    obs = VECTOR_ENVS[env_id][1]
    if obs == 4:
        return rng.uniform(-0.05, 0.05, (n, 4)).astype(np.float32)
    return np.stack([rng.uniform(-0.6, -0.4, n), np.zeros(n)], 1).astype(np.float32)


def philox_reset_draws(env_id: str, seed: int, n: int) -> np.ndarray:
    """The reset formula of ``vec_classic_reset`` at step counter 0 on the host Philox draw
    (stream = env index, counter = 1), fp32 constants combined in fp64: [n, obs]."""
    from .actor_oracle import uniform4

    obs = VECTOR_ENVS[env_id][1]
    f = lambda v: float(np.float32(v))
    out = np.zeros((n, obs))
    for e in range(n):
        u = uniform4(seed, e, 1)
        if obs == 4:
            out[e] = [f(-0.05) + f(0.1) * float(u[k]) for k in range(4)]
        else:
            out[e] = [f(-0.6) + f(0.2) * float(u[0]), 0.0]
    return out


def host_episodes(model, env_id: str, starts: np.ndarray, limit: int | None = None) -> dict:
    """Greedy episodes of the fp64 net from ``starts`` (states carried in fp32): lengths, end
    kinds (1 terminal / 2 time limit), action counts, steps whose next state lies within
    ``NEAR`` of a threshold, and the smallest relative top-2 Q gap."""
    limit = VECTOR_ENVS[env_id][3] if limit is None else limit
    net, env = fp64(model), envs.make(env_id)
    lengths, ended, near, steps, gap = [], [], 0, 0, np.inf
    acts = np.zeros(model.num_actions, dtype=np.int64)
    for s in starts:
        s = np.asarray(s, dtype=np.float32)
        for t in range(1, limit + 1):
            with torch.no_grad():
                q = net(torch.from_numpy(s.astype(np.float64))[None]).numpy()[0]
            a = int(q.argmax())
            acts[a] += 1
            top = np.sort(q)
            gap = min(gap, (top[-1] - top[-2]) / np.abs(q).max())
            nxt, term, margin = host_step(env, s, a)
            s = nxt.astype(np.float32)
            steps += 1
            near += margin <= NEAR
            if term or t >= limit:
                break
        lengths.append(t)
        ended.append(1 if term else 2)
    return {"lengths": lengths, "ended": ended, "actions": acts, "near": int(near), "steps": steps,
            "min_gap": float(gap)}
