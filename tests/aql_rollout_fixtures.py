"""Weights and seeds shared by the AQL rollout tests (host self-checks and GPU tests), and a host
model of greedy CartPole episodes (fp64 eval-mode ``AQL``, ``envs/classic.py``, host RNG).

``set_params`` fills every parameter and noise buffer of an ``AQL`` from one CPU generator, so
the host checks and the GPU engines hold the same numbers: weights U(-1, 1) / sqrt(fan_in),
non-zero biases, and non-zero NoisyNet sigma AND epsilon -- evaluation must use the means, and
a kernel that wrongly applies the noise is then caught."""
from __future__ import annotations

import numpy as np
import torch

from apex_amd import envs
from apex_amd.models.aql import AQL

CARTPOLE_KW = dict(propose_sample=3)            # natural T = 2 uniform (both actions) + 3 proposed
CARTPOLE_SEEDS = (1234, 5)                      # the env seeds of the GPU CartPole tests
NEAR = 1e-4   # a next state this close to a termination threshold is not compared for its terminal flag


def set_params(model: AQL, seed: int = 3) -> None:
    g = torch.Generator(device="cpu").manual_seed(seed)
    u = lambda shape: torch.rand(shape, generator=g) * 2 - 1  # noqa: E731
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "sigma" in name:
                v = torch.full(p.shape, 0.3)
            elif p.dim() == 1:
                v = 0.2 * u(p.shape)
            else:
                v = u(p.shape) / float(p.shape[1]) ** 0.5
            p.copy_(v.to(device=p.device, dtype=p.dtype))
        for lin in (model.q.advantage1, model.q.advantage2):
            for b in (lin.weight_epsilon, lin.bias_epsilon):
                b.copy_(u(b.shape).to(device=b.device, dtype=b.dtype))


def host_cartpole_model() -> AQL:
    m = AQL(envs.make("CartPole-v0"), device="cpu", **CARTPOLE_KW)
    set_params(m)
    m = m.double()
    m.q.eval()
    return m


def host_cartpole_episodes(model: AQL, seed: int, episodes: int, limit: int = 200):
    """Greedy episodes on the host: (lengths, steps, steps whose next state is within NEAR of a
    termination threshold)."""
    rng = np.random.RandomState(seed)
    env = envs.make("CartPole-v0").unwrapped
    env.seed(seed)
    qn, T = model.q, model.total_sample
    lengths, steps, near = [], 0, 0
    for _ in range(episodes):
        s = env.reset()
        for t in range(limit):
            with torch.no_grad():
                st = torch.as_tensor(np.asarray(s, np.float32), dtype=torch.float64)[None]
                logits = model.proposal.dist_feature(qn.embedding_feature(st))[0]
                p = torch.softmax(logits, 0).numpy()
                cand = np.concatenate([rng.permutation(2), rng.choice(2, size=T - 2, p=p / p.sum())])
                a_out = qn.action_out(torch.as_tensor(cand, dtype=torch.float64).reshape(T, 1)).reshape(1, T, -1)
                q_f = qn.q_feature(st).repeat(1, T).reshape(1, T, -1)
                q = qn.forward(torch.relu(torch.cat([a_out, q_f], dim=2))).reshape(T)
            s, _, d, _ = env.step(int(cand[int(torch.argmax(q))]))
            steps += 1
            near += min(abs(abs(s[0]) - env.x_threshold), abs(abs(s[2]) - env.theta_threshold_radians)) < NEAR
            if d:
                break
        lengths.append(t + 1)
    return lengths, steps, near
