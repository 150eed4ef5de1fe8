"""Shared pieces of the host-env tests: a shortened emulator, twin pipelines and the fp64 host
oracle of the ingest kernel's warp."""
import numpy as np

from apex_amd.envs.core import Wrapper, make
from apex_amd.envs.preprocess import GREY, AtariPreprocess, PreprocessSpec, area_weights
from apex_amd.envs.raw_vector import RawAtariVector


class Shortened(Wrapper):
    """The synthetic emulator with scripted bad luck, so a short test sees life losses and game
    overs: every ``life_every`` raw frames a life is taken (games with lives; the last one ends
    the game), and a game without lives ends after ``over_at`` raw frames.  Both land at any
    phase of the repeat window."""

    def __init__(self, env, life_every=23, over_at=61):
        super().__init__(env)
        self.life_every, self.over_at = life_every, over_at
        self.n = 0

    def reset(self, **kw):
        self.n = 0
        return self.env.reset(**kw)

    def step(self, action):
        obs, r, done, info = self.env.step(action)
        self.n += 1
        raw = self.env.unwrapped
        if raw.lives > 0 and self.n % self.life_every == 0:
            raw.lives -= 1
            done = done or raw.lives <= 0
        elif raw.lives == 0 and self.n >= self.over_at:
            done = True
        return obs, r, done, info


def twins(game: str, n: int, seed: int, spec: PreprocessSpec = PreprocessSpec(), shortened: bool = True,
          life_every: int = 23):
    """(RawAtariVector, AtariPreprocess) over separately built, equally seeded emulators."""
    env_id = f"{game}NoFrameskip-v4"
    build = (lambda: Shortened(make(env_id), life_every)) if shortened else (lambda: make(env_id))
    raw, ref = RawAtariVector([build() for _ in range(n)], spec), AtariPreprocess([build() for _ in range(n)], spec)
    for p in (raw, ref):
        p.seed(seed)
        p.fixed_noops = [3 + i for i in range(n)]
    return raw, ref


def warp_pre(pair: np.ndarray) -> np.ndarray:
    """fp64 pre-rounding values [84, 84] (h, w) of one ``[2, H, W, 3]`` pair: AreaResize's
    arithmetic on the pooled frame."""
    H, W = pair.shape[1:3]
    grey = np.maximum(pair[0], pair[1]).astype(np.float64) @ GREY
    return area_weights(84, H) @ grey @ area_weights(84, W).T


def warp_plane(pair: np.ndarray) -> np.ndarray:
    """The ring plane of a pair: rounded, clamped, transposed (``channels_first``), flat [7056]."""
    out = np.clip(np.rint(warp_pre(pair)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(out.T).reshape(-1)


def near_half(pre: np.ndarray, tol: float = 1e-9) -> np.ndarray:
    """Mask of pre-rounding values within ``tol`` of a half-integer (the rounding ties)."""
    return np.abs(pre - np.floor(pre) - 0.5) <= tol
