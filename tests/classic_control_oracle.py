"""Acrobot-v1 and MountainCar-v0 on the host - TEST INFRASTRUCTURE for tests/test_classic_control_cpu.py and
tests/test_classic_control_gpu.py.

* the fp32 restatements of the device envs (csrc/orl_env.h: acrobot_step / acrobot_reset, mountaincar_pre /
  mountaincar_post / mountaincar_reset - the same expression order, explicit fmaf emulated exactly) and float64
  transcriptions of gymnasium's two steps (classic_control/acrobot.py with ``book_or_nips = "book"``,
  classic_control/mountain_car.py) to check them against;
* the host Philox reset states, keyed (seed, env, episode) as on the device;
* ``AcrobotEnvOracle`` / ``MountainCarEnvOracle``: the vectorised envs with the device envs' semantics, duck-typed like
  ``oracle.ppo_oracle.CartPoleEnvOracle`` so that ``oracle.cpu_trainer.CPUTrainer(obs_dim=6 | 2, n_actions=3, env=...)``
  drives them.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import philox as px

f32 = np.float32
ACRO_PI, ACRO_2PI = f32(math.pi), f32(2.0 * math.pi)
ACRO_MAX_VEL_1, ACRO_MAX_VEL_2 = f32(4.0 * math.pi), f32(9.0 * math.pi)
ACROBOT_KEY, MOUNTAINCAR_KEY = 0xAC40B000, 0x3C4A0000
ACROBOT_STATE_W, MOUNTAINCAR_STATE_W = 6, 4
ACROBOT_LIMIT, MOUNTAINCAR_LIMIT = 500, 200


def _fma32(a, b, c):
    """fmaf in float32: the product of two float32 values is exact in float64, so one float64 add and one rounding to
    float32 give the fused result (double rounding aside - a last-bit difference at most)."""
    return (np.asarray(a, f32).astype(np.float64) * np.asarray(b, f32).astype(np.float64)
            + np.asarray(c, f32).astype(np.float64)).astype(f32)


# ============================================================================================ Acrobot-v1
def acrobot_dsdt_f32(s, a):
    """csrc/orl_env.h acrobot_dsdt: s [N, 4], a [N] torques -> [N, 4] derivatives (fp32, the device's order)."""
    s = np.asarray(s, f32)
    th1, th2, d1v, d2v = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    s2, c2 = np.sin(th2).astype(f32), np.cos(th2).astype(f32)
    s1 = np.sin(th1).astype(f32)
    s12 = np.sin((th1 + th2).astype(f32)).astype(f32)
    d1 = (f32(3.5) + c2).astype(f32)
    d2 = _fma32(f32(0.5), c2, f32(1.25))
    phi2 = (f32(4.9) * s12).astype(f32)
    w = _fma32(d2v, d2v, ((f32(2.0) * d2v).astype(f32) * d1v).astype(f32))
    m05s2 = (f32(-0.5) * s2).astype(f32)
    phi1 = _fma32(m05s2, w, _fma32(f32(14.7), s1, phi2))
    r = (d2 / d1).astype(f32)
    num = (_fma32(m05s2, (d1v * d1v).astype(f32), _fma32(r, phi1, np.asarray(a, f32))) - phi2).astype(f32)
    dd2 = (num / _fma32(-d2, r, f32(1.25))).astype(f32)
    dd1 = (-_fma32(d2, dd2, phi1) / d1).astype(f32)
    return np.stack([d1v, d2v, dd1, dd2], axis=-1).astype(f32)


def acrobot_wrap_f32(x):
    x = np.asarray(x, f32).copy()
    for _ in range(16):
        x = np.where(x > ACRO_PI, (x - ACRO_2PI).astype(f32), x)
    for _ in range(16):
        x = np.where(x < -ACRO_PI, (x + ACRO_2PI).astype(f32), x)
    return x.astype(f32)


def acrobot_obs_f32(state):
    s = np.asarray(state, f32)
    return np.stack([np.cos(s[:, 0]), np.sin(s[:, 0]), np.cos(s[:, 1]), np.sin(s[:, 1]), s[:, 2], s[:, 3]],
                    axis=-1).astype(f32)


def acrobot_terminal_f32(state):
    s = np.asarray(state, f32)
    return (-np.cos(s[:, 0]).astype(f32) - np.cos((s[:, 1] + s[:, 0]).astype(f32)).astype(f32)) > f32(1.0)


def acrobot_step_f32(state, action):
    """gymnasium Acrobot-v1 step in float32 with the device's expression order (csrc/orl_env.h acrobot_step).
    state [N, 4] = (th1, th2, dth1, dth2), action [N] in {0, 1, 2}.  Returns (next state, obs [N, 6], terminated [N],
    reward [N]: -1, or 0 on the terminating step)."""
    s = np.asarray(state, f32)
    a = np.clip(np.asarray(action).reshape(-1).astype(np.int64), 0, 2)
    torque = (a - 1).astype(f32)
    dt, dt2, dt6 = f32(0.2), f32(0.1), f32(0.2 / 6.0)
    k1 = acrobot_dsdt_f32(s, torque)
    k2 = acrobot_dsdt_f32(_fma32(dt2, k1, s), torque)
    k3 = acrobot_dsdt_f32(_fma32(dt2, k2, s), torque)
    k4 = acrobot_dsdt_f32(_fma32(dt, k3, s), torque)
    acc = (_fma32(f32(2.0), k3, _fma32(f32(2.0), k2, k1)) + k4).astype(f32)
    y = _fma32(dt6, acc, s)
    nxt = np.stack([acrobot_wrap_f32(y[:, 0]), acrobot_wrap_f32(y[:, 1]),
                    np.clip(y[:, 2], -ACRO_MAX_VEL_1, ACRO_MAX_VEL_1), np.clip(y[:, 3], -ACRO_MAX_VEL_2, ACRO_MAX_VEL_2)],
                   axis=-1).astype(f32)
    term = acrobot_terminal_f32(nxt)
    return nxt, acrobot_obs_f32(nxt), term, np.where(term, f32(0.0), f32(-1.0)).astype(f32)


def _acrobot_dsdt_f64(s_aug):
    """gymnasium acrobot.py AcrobotEnv._dsdt (book dynamics), transcribed."""
    m1 = m2 = 1.0
    l1 = 1.0
    lc1 = lc2 = 0.5
    I1 = I2 = 1.0
    g = 9.8
    a = s_aug[-1]
    theta1, theta2, dtheta1, dtheta2 = s_aug[:-1]
    d1 = m1 * lc1 ** 2 + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * math.cos(theta2)) + I1 + I2
    d2 = m2 * (lc2 ** 2 + l1 * lc2 * math.cos(theta2)) + I2
    phi2 = m2 * lc2 * g * math.cos(theta1 + theta2 - math.pi / 2.0)
    phi1 = (-m2 * l1 * lc2 * dtheta2 ** 2 * math.sin(theta2) - 2 * m2 * l1 * lc2 * dtheta2 * dtheta1 * math.sin(theta2)
            + (m1 * lc1 + m2 * l1) * g * math.cos(theta1 - math.pi / 2) + phi2)
    ddtheta2 = (a + d2 / d1 * phi1 - m2 * l1 * lc2 * dtheta1 ** 2 * math.sin(theta2) - phi2) / (
        m2 * lc2 ** 2 + I2 - d2 ** 2 / d1)
    ddtheta1 = -(d2 * ddtheta2 + phi1) / d1
    return np.array([dtheta1, dtheta2, ddtheta1, ddtheta2, 0.0])


def _wrap_f64(x, m, M):
    diff = M - m
    while x > M:
        x = x - diff
    while x < m:
        x = x + diff
    return x


def acrobot_step_f64(state, action):
    """gymnasium AcrobotEnv.step transcribed in float64 (rk4 over [0, dt], wrap, bound, _terminal): returns
    (next state [4], terminated, reward)."""
    s_aug = np.append(np.asarray(state, np.float64), [-1.0, 0.0, 1.0][int(action)])
    dt = 0.2
    k1 = _acrobot_dsdt_f64(s_aug)
    k2 = _acrobot_dsdt_f64(s_aug + dt / 2.0 * k1)
    k3 = _acrobot_dsdt_f64(s_aug + dt / 2.0 * k2)
    k4 = _acrobot_dsdt_f64(s_aug + dt * k3)
    ns = (s_aug + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4))[:4]
    ns[0] = _wrap_f64(ns[0], -math.pi, math.pi)
    ns[1] = _wrap_f64(ns[1], -math.pi, math.pi)
    ns[2] = min(max(ns[2], -4 * math.pi), 4 * math.pi)
    ns[3] = min(max(ns[3], -9 * math.pi), 9 * math.pi)
    term = bool(-math.cos(ns[0]) - math.cos(ns[1] + ns[0]) > 1.0)
    return ns, term, (0.0 if term else -1.0)


def acrobot_reset_state(seed: int, env: np.ndarray, episode: np.ndarray) -> np.ndarray:
    """(th1, th2, dth1, dth2) of episode ``episode`` of env ``env``: U(-0.1, 0.1) each from Philox keyed
    (seed, env, episode) under the Acrobot key (csrc/orl_env.h acrobot_reset)."""
    r = px.philox4x32_10(seed, np.asarray(env).astype(np.uint32), ACROBOT_KEY, np.asarray(episode).astype(np.uint32), 0)
    return np.stack([_fma32(px.u01(x), f32(0.2), f32(-0.1)) for x in r], axis=-1).astype(f32)


# ============================================================================================ MountainCar-v0
def mountaincar_step_f32(state, action):
    """gymnasium MountainCar-v0 step in float32 with the device's expression order (mountaincar_pre / _post).
    state [N, 2] = (position, velocity), action [N] in {0, 1, 2}.  Returns (next state = obs, terminated, reward)."""
    s = np.asarray(state, f32)
    p, v = s[:, 0], s[:, 1]
    a = np.clip(np.asarray(action).reshape(-1).astype(np.int64), 0, 2)
    pre = (np.cos((f32(3.0) * p).astype(f32)).astype(f32) * f32(-0.0025)).astype(f32)
    v = (v + _fma32((a - 1).astype(f32), f32(0.001), pre)).astype(f32)
    v = np.clip(v, f32(-0.07), f32(0.07)).astype(f32)
    p = np.clip((p + v).astype(f32), f32(-1.2), f32(0.6)).astype(f32)
    v = np.where((p == f32(-1.2)) & (v < 0), f32(0.0), v).astype(f32)
    term = (p >= f32(0.5)) & (v >= 0)
    nxt = np.stack([p, v], axis=-1).astype(f32)
    return nxt, term, np.full(p.shape, -1.0, f32)


def mountaincar_step_f64(state, action):
    """gymnasium MountainCarEnv.step transcribed in float64: (next state [2], terminated, reward)."""
    position, velocity = float(state[0]), float(state[1])
    velocity += (int(action) - 1) * 0.001 + math.cos(3 * position) * (-0.0025)
    velocity = float(np.clip(velocity, -0.07, 0.07))
    position += velocity
    position = float(np.clip(position, -1.2, 0.6))
    if position == -1.2 and velocity < 0:
        velocity = 0
    term = bool(position >= 0.5 and velocity >= 0)
    return np.array([position, velocity]), term, -1.0


def mountaincar_reset_state(seed: int, env: np.ndarray, episode: np.ndarray) -> np.ndarray:
    """(position, velocity) of episode ``episode`` of env ``env``: position U(-0.6, -0.4), velocity 0."""
    x, _, _, _ = px.philox4x32_10(seed, np.asarray(env).astype(np.uint32), MOUNTAINCAR_KEY,
                                  np.asarray(episode).astype(np.uint32), 0)
    p = _fma32(px.u01(x), f32(0.2), f32(-0.6))
    return np.stack([p, np.zeros_like(p)], axis=-1).astype(f32)


# ============================================================================================ vectorised envs
class _ClassicControlOracle:
    """done = terminated or truncated (``episode_limit`` steps), auto-reset to the Philox start state of
    (seed, env, episode) with the observation of the NEW episode returned.  Duck-typed like CartPoleEnvOracle."""

    def __init__(self, n_envs, seed, episode_limit):
        self.N, self.seed, self.limit = n_envs, seed, episode_limit
        self.reset()

    def reset(self):
        self.episode = np.zeros(self.N, np.int64)
        self.steps = np.zeros(self.N, np.int64)
        self.state = self._reset_state(self.seed, np.arange(self.N), self.episode)
        return self._obs(self.state)[:, None, :]

    def step(self, actions):
        a = np.asarray(actions).reshape(self.N).astype(np.int64)
        nxt, obs, term, rew = self._step(self.state, a)
        self.steps = self.steps + 1
        done = term | (self.steps >= self.limit)
        self.episode = np.where(done, self.episode + 1, self.episode)
        fresh = self._reset_state(self.seed, np.arange(self.N), self.episode)
        self.state = np.where(done[:, None], fresh, nxt).astype(f32)
        obs = np.where(done[:, None], self._obs(fresh), obs).astype(f32)
        self.steps = np.where(done, 0, self.steps)
        return obs[:, None, :], rew.reshape(self.N, 1, 1), done[:, None], [{} for _ in range(self.N)]


class AcrobotEnvOracle(_ClassicControlOracle):
    def __init__(self, n_envs, seed, episode_limit=ACROBOT_LIMIT):
        super().__init__(n_envs, seed, episode_limit)

    _reset_state = staticmethod(acrobot_reset_state)
    _obs = staticmethod(acrobot_obs_f32)

    @staticmethod
    def _step(state, a):
        return acrobot_step_f32(state, a)


class MountainCarEnvOracle(_ClassicControlOracle):
    def __init__(self, n_envs, seed, episode_limit=MOUNTAINCAR_LIMIT):
        super().__init__(n_envs, seed, episode_limit)

    _reset_state = staticmethod(mountaincar_reset_state)

    @staticmethod
    def _obs(state):
        return np.asarray(state, f32).copy()

    @staticmethod
    def _step(state, a):
        nxt, term, rew = mountaincar_step_f32(state, a)
        return nxt, nxt.copy(), term, rew
