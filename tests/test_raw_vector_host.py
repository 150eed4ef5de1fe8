"""CPU tests of the host-env front end: ``RawAtariVector`` against its twin ``AtariPreprocess``
(same emulators, seeds and actions: the max of every pair, warped on the host, is the twin's
newest frame), the pair pool's two modes, the vector-env protocol, and the ingest kernel's tap
tables against ``area_weights``."""
import numpy as np
import pytest

from apex_amd.envs.preprocess import AreaResize, PreprocessSpec, RepeatPool, area_weights, channels_first
from apex_amd.envs.raw_vector import PairPool, RawAtariVector

from .host_env_util import twins


def _newest(pair, resize):
    return channels_first(resize(np.maximum(pair[0], pair[1])))


@pytest.mark.parametrize("reference_pool", [True, False])
@pytest.mark.parametrize("game", ["Seaquest", "Pong"])
def test_raw_vector_twins_the_host_pipeline(game, reference_pool):
    E, T = 3, 90
    spec = PreprocessSpec(clip_rewards=False, reference_pool=reference_pool)
    raw, ref = twins(game, E, seed=11, spec=spec)
    assert raw.n_actions == (18 if game == "Seaquest" else 6) and raw.fire
    resize = AreaResize(raw.raw_shape[:2])
    out = np.zeros((E, 2) + raw.raw_shape, np.uint8)
    raw.reset(out)
    obs = ref.reset()
    for i in range(E):
        assert np.array_equal(_newest(out[i], resize)[0], obs[i][-1])
    rng = np.random.default_rng(0)
    life_losses = game_overs = 0
    for t in range(T):
        acts = rng.integers(0, raw.n_actions, E)
        r, d = raw.step(acts, out)
        obs, r_ref, d_ref, _ = ref.step(acts)  # (clip_rewards off: the unclipped window sum)
        assert r.dtype == np.float64 and d.dtype == bool
        assert np.array_equal(r, r_ref) and np.array_equal(d, d_ref), t
        for i in range(E):
            if d[i]:
                over = ref.ledgers[i].game_over
                game_overs += over
                life_losses += not over
                start = ref.reset_one(i)       # the raw vector restarted env i by itself
                assert np.array_equal(_newest(out[i], resize)[0], start[-1]), (t, i)
                assert all(np.array_equal(start[c], start[-1]) for c in range(4))
            else:
                assert np.array_equal(_newest(out[i], resize)[0], obs[i][-1]), (t, i)
    assert game_overs > 0
    if game == "Seaquest":
        assert life_losses > 0


def _stepper(dones):
    it, k = iter(dones), [0]

    def step(_a):
        k[0] += 1
        return np.full((2, 2, 3), k[0], dtype=np.uint8), 1.0, next(it), {}
    return step


@pytest.mark.parametrize("reference", [True, False])
def test_pair_pool_max_is_the_repeat_pool(reference):
    """Window 1 runs to its end, window 2 ends early at each of its four steps: the max of the
    pair is RepeatPool's frame -- with the reference pool, slots of an OLDER window."""
    for early in range(4):
        dones = [False] * 4 + [False] * early + [True]
        pair, pool = PairPool(4, reference), RepeatPool(4, reference)
        s_pair, s_pool = _stepper(dones), _stepper(dones)
        for _ in range(2):
            p, r, d, _ = pair.run(s_pair, 0)
            f, r2, d2, _ = pool.run(s_pool, 0)
            assert p.shape == (2, 2, 2, 3) and np.array_equal(p.max(axis=0), f) and (r, d) == (r2, d2)
        assert d
        if reference and early < 2:
            assert int(p.max()) == 4              # frames 3 and 4 of window 1
        if not reference and early == 0:
            assert int(p[0].max()) == int(p[1].max()) == 5   # the window's only frame, twice


def test_single_frame_start_is_written_twice_and_protocol():
    from apex_amd.envs.core import make

    spec = PreprocessSpec(fire_reset=False, episode_life=False)   # the start is the no-op start's last frame
    vec = RawAtariVector([make("PongNoFrameskip-v4") for _ in range(2)], spec)
    vec.seed(3)
    vec.fixed_noops = [2, 5]
    assert len(vec) == 2 and vec.raw_shape == (210, 160, 3) and vec.n_actions == 6
    assert callable(vec.reset) and callable(vec.step)
    out = np.full((2, 2, 210, 160, 3), 7, np.uint8)
    vec.reset(out)
    assert np.array_equal(out[:, 0], out[:, 1]) and out.max() > 7
    r, d = vec.step([0, 1], out)
    assert r.shape == (2,) and d.shape == (2,) and not np.array_equal(out[:, 0], out[:, 1])
    with pytest.raises(ValueError):
        vec.step([0, 1], np.zeros((2, 210, 160, 3), np.uint8))


@pytest.mark.parametrize("H,W", [(210, 160), (250, 160), (84, 84)])
def test_tap_tables_rebuild_area_weights_exactly(H, W):
    from apex_amd.engine.host_env import TAP_WIDTH, dense_from_taps, tap_tables

    for n in (H, W):
        first, count, weight = tap_tables(n)
        assert first.dtype == count.dtype == np.int32 and weight.shape == (84, TAP_WIDTH)
        assert count.min() >= 1 and (first + count <= n).all()
        assert np.array_equal(dense_from_taps(first, count, weight, n), area_weights(84, n))


def test_tap_tables_reject_what_the_kernel_cannot_do():
    from apex_amd.engine.host_env import Ingest, tap_tables

    with pytest.raises(ValueError):
        tap_tables(83)
    with pytest.raises(ValueError):
        tap_tables(84 * 9)            # 9 or more taps per output pixel: wider than the table
    with pytest.raises(ValueError):
        tap_tables(210, width=2)
    for H, W in [(80, 160), (210, 64)]:  # the launcher's own check comes before any device work
        with pytest.raises(ValueError):
            Ingest(3, H, W, 7056, 16, True, "cpu")
