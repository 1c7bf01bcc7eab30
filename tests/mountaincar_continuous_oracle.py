"""MountainCarContinuous-v0 on the host - TEST INFRASTRUCTURE for tests/test_mountaincar_continuous_cpu.py and
tests/test_mountaincar_continuous_gpu.py.

* the fp32 restatement of the device env (csrc/orl_env.h: mountaincar_pre / mountaincar_cont_post /
  mountaincar_cont_reward / mountaincar_cont_reset - the same expression order, explicit fmaf emulated exactly) and a
  float64 transcription of gymnasium's step (classic_control/continuous_mountain_car.py, the state rounded to float32
  after every step) to check it against;
* the host Philox reset states, keyed (seed, env, episode) as on the device;
* ``MountainCarContinuousEnvOracle``: the vectorised env with the device env's semantics, duck-typed like
  ``tests.classic_control_oracle.MountainCarEnvOracle`` so that ``tests.pendulum_oracle.GaussianCPUTrainer(obs_dim=2,
  n_actions=1, env=...)`` drives it.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import philox as px

f32 = np.float32
MOUNTAINCAR_CONT_KEY = 0x3CC40000
MOUNTAINCAR_CONT_STATE_W = 4
MOUNTAINCAR_CONT_LIMIT = 999
GOAL = f32(0.45)
POWER = f32(0.0015)


def _fma32(a, b, c):
    """fmaf in float32: the product of two float32 values is exact in float64, so one float64 add and one rounding to
    float32 give the fused result (double rounding aside - a last-bit difference at most)."""
    return (np.asarray(a, f32).astype(np.float64) * np.asarray(b, f32).astype(np.float64)
            + np.asarray(c, f32).astype(np.float64)).astype(f32)


def mountaincar_pre_f32(p):
    """csrc/orl_env.h mountaincar_pre: the gravity term cos(3 p) * -0.0025 (two roundings)."""
    p = np.asarray(p, f32)
    return (np.cos((f32(3.0) * p).astype(f32)).astype(f32) * f32(-0.0025)).astype(f32)


def mountaincar_cont_post_f32(state, pre, action):
    """csrc/orl_env.h mountaincar_cont_post: state [N, 2], pre [N], action [N] (unclipped) -> (next state, terminated)."""
    s = np.asarray(state, f32)
    p, v = s[:, 0], s[:, 1]
    force = np.clip(np.asarray(action, f32).reshape(-1), f32(-1.0), f32(1.0)).astype(f32)
    v = (v + _fma32(force, POWER, pre)).astype(f32)
    v = np.clip(v, f32(-0.07), f32(0.07)).astype(f32)
    p = np.clip((p + v).astype(f32), f32(-1.2), f32(0.6)).astype(f32)
    v = np.where((p == f32(-1.2)) & (v < 0), f32(0.0), v).astype(f32)
    term = (p >= GOAL) & (v >= 0)
    return np.stack([p, v], axis=-1).astype(f32), term


def mountaincar_cont_reward_f32(term, action):
    """csrc/orl_env.h mountaincar_cont_reward: (100 if terminated else 0) - (a * a) * 0.1 on the UNCLIPPED action."""
    a = np.asarray(action, f32).reshape(-1)
    cost = ((a * a).astype(f32) * f32(0.1)).astype(f32)
    return (np.where(term, f32(100.0), f32(0.0)) - cost).astype(f32)


def mountaincar_cont_step_f32(state, action):
    """gymnasium MountainCarContinuous-v0 step in float32 with the device's expression order.  state [N, 2] =
    (position, velocity), action [N] float (unclipped).  Returns (next state = obs, terminated, reward)."""
    s = np.asarray(state, f32)
    nxt, term = mountaincar_cont_post_f32(s, mountaincar_pre_f32(s[:, 0]), action)
    return nxt, term, mountaincar_cont_reward_f32(term, action)


def mountaincar_cont_step_f64(state, action):
    """gymnasium Continuous_MountainCarEnv.step transcribed in float64, the state rounded to float32 at the end as
    gymnasium does (``np.array([position, velocity], dtype=np.float32)``): (next state [2] float32, terminated,
    reward)."""
    position, velocity = float(state[0]), float(state[1])
    a = float(action)
    force = min(max(a, -1.0), 1.0)
    velocity += force * 0.0015 - 0.0025 * math.cos(3 * position)
    if velocity > 0.07:
        velocity = 0.07
    if velocity < -0.07:
        velocity = -0.07
    position += velocity
    if position > 0.6:
        position = 0.6
    if position < -1.2:
        position = -1.2
    if position == -1.2 and velocity < 0:
        velocity = 0
    term = bool(position >= 0.45 and velocity >= 0.0)
    reward = 0.0
    if term:
        reward = 100.0
    reward -= math.pow(a, 2) * 0.1
    return np.array([position, velocity], dtype=np.float32), term, reward


def mountaincar_cont_reset_state(seed: int, env: np.ndarray, episode: np.ndarray) -> np.ndarray:
    """(position, velocity) of episode ``episode`` of env ``env``: position U(-0.6, -0.4), velocity 0, from Philox keyed
    (seed, env, episode) under MountainCarContinuous's own key (csrc/orl_env.h mountaincar_cont_reset)."""
    x, _, _, _ = px.philox4x32_10(seed, np.asarray(env).astype(np.uint32), MOUNTAINCAR_CONT_KEY,
                                  np.asarray(episode).astype(np.uint32), 0)
    p = _fma32(px.u01(x), f32(0.2), f32(-0.6))
    return np.stack([p, np.zeros_like(p)], axis=-1).astype(f32)


class MountainCarContinuousEnvOracle:
    """Vectorised MountainCarContinuous-v0 with the device env's semantics: mountaincar_cont_step_f32, done =
    terminated or truncated (``episode_limit`` steps), auto-reset to the Philox start state of (seed, env, episode)
    with the observation of the NEW episode returned.  Actions are floats, used unclipped for the reward."""

    def __init__(self, n_envs, seed, episode_limit=MOUNTAINCAR_CONT_LIMIT):
        self.N, self.seed, self.limit = n_envs, seed, episode_limit
        self.reset()

    def reset(self):
        self.episode = np.zeros(self.N, np.int64)
        self.steps = np.zeros(self.N, np.int64)
        self.state = mountaincar_cont_reset_state(self.seed, np.arange(self.N), self.episode)
        return self.state.copy()[:, None, :]

    def step(self, actions):
        a = np.asarray(actions, f32).reshape(self.N)
        nxt, term, rew = mountaincar_cont_step_f32(self.state, a)
        self.steps = self.steps + 1
        done = term | (self.steps >= self.limit)
        self.episode = np.where(done, self.episode + 1, self.episode)
        fresh = mountaincar_cont_reset_state(self.seed, np.arange(self.N), self.episode)
        self.state = np.where(done[:, None], fresh, nxt).astype(f32)
        self.steps = np.where(done, 0, self.steps)
        return self.state.copy()[:, None, :], rew.reshape(self.N, 1, 1), done[:, None], [{} for _ in range(self.N)]
