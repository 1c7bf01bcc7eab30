"""Pendulum-v1 on the host - TEST INFRASTRUCTURE for tests/test_pendulum_cpu.py and tests/test_pendulum_gpu.py.

* the fp32 restatement of the device env (csrc/orl_env.h: pendulum_reset / pendulum_pre / pendulum_post, the same
  expression order, explicit fmaf emulated exactly) and a float64 transcription of gymnasium's step
  (classic_control/pendulum.py) to check it against;
* ``PendulumEnvOracle``: the vectorised env with the device env's semantics, duck-typed like
  ``oracle.ppo_oracle.CartPoleEnvOracle``;
* ``GaussianCPUTrainer``: ``oracle.cpu_trainer.CPUTrainer`` (the CPU port of the reference's collect + PPO update) with a
  DiagGaussian policy head - ``Normal(mean, exp(logstd))`` sampling, the unclipped sample stored with its log-prob - and a
  configurable discount.  Every numeric definition comes from ``oracle.ppo_oracle`` (pinned against the reference).
"""
from __future__ import annotations

import math
import time
from typing import Dict

import numpy as np
import torch

from oracle import philox as px
from oracle import ppo_oracle as po
from oracle.cpu_trainer import CPUReplayData, CPUTrainer

PEND_PI, PEND_2PI = np.float32(math.pi), np.float32(2.0 * math.pi)


def _fma32(a, b, c):
    """fmaf in float32: the product of two float32 values is exact in float64, so one float64 add and one rounding to
    float32 give the fused result (double rounding aside - a last-bit difference at most)."""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def pendulum_angle_normalize_f32(x):
    """gymnasium's ``((x + pi) % (2 pi)) - pi`` with Python's floored modulo, as the device computes it: fmodf (truncated,
    exact) plus 2 pi where the remainder is negative."""
    f = np.float32
    r = np.fmod((np.asarray(x, f) + PEND_PI).astype(f), PEND_2PI).astype(f)
    r = np.where(r < 0, (r + PEND_2PI).astype(f), r).astype(f)
    return (r - PEND_PI).astype(f)


def pendulum_wrap_f32(th):
    th = np.asarray(th, np.float32)
    return np.where(th >= PEND_PI, th - PEND_2PI, np.where(th < -PEND_PI, th + PEND_2PI, th)).astype(np.float32)


def pendulum_obs_f32(state):
    s = np.asarray(state, np.float32)
    return np.stack([np.cos(s[:, 0]), np.sin(s[:, 0]), s[:, 1]], axis=-1).astype(np.float32)


def pendulum_step_f32(state: np.ndarray, action: np.ndarray):
    """gymnasium Pendulum-v1 step (classic_control/pendulum.py step()) in float32 with the device's expression order
    (csrc/orl_env.h pendulum_pre / pendulum_post, explicit fmaf) and its one deviation: th wrapped to [-pi, pi) after
    the step.  state [N, 2] = (th, thdot), action [N] (unclipped).  Returns (next state [N, 2], obs [N, 3], reward [N])."""
    f = np.float32
    s = np.asarray(state, f)
    th, thdot = s[:, 0], s[:, 1]
    u = np.clip(np.asarray(action, f).reshape(-1), f(-2.0), f(2.0)).astype(f)
    an = pendulum_angle_normalize_f32(th)
    grav = (f(15.0) * np.sin(th).astype(f)).astype(f)
    cost0 = _fma32((f(0.1) * thdot).astype(f), thdot, (an * an).astype(f))
    cost = _fma32((f(0.001) * u).astype(f), u, cost0)
    acc = _fma32(f(3.0), u, grav)
    ndot = np.clip(_fma32(acc, f(0.05), thdot), f(-8.0), f(8.0)).astype(f)
    nth = pendulum_wrap_f32(_fma32(ndot, f(0.05), th))
    nxt = np.stack([nth, ndot], axis=-1).astype(f)
    return nxt, pendulum_obs_f32(nxt), (-cost).astype(f)


def pendulum_step_f64(th, thdot, u):
    """The gymnasium step transcribed in float64 (no wrap): (new th, new thdot, reward) - the reference the fp32
    restatement is checked against."""
    th, thdot = np.float64(th), np.float64(thdot)
    u = np.clip(np.float64(u), -2.0, 2.0)
    an = ((th + np.pi) % (2 * np.pi)) - np.pi
    cost = an ** 2 + 0.1 * thdot ** 2 + 0.001 * (u ** 2)
    ndot = np.clip(thdot + (3 * 10.0 / (2 * 1.0) * np.sin(th) + 3.0 / (1.0 * 1.0 ** 2) * u) * 0.05, -8.0, 8.0)
    return th + ndot * 0.05, ndot, -cost


def pendulum_reset_state(seed: int, env: np.ndarray, episode: np.ndarray) -> np.ndarray:
    """(th, thdot) of episode ``episode`` of env ``env``: th ~ U(-pi, pi), thdot ~ U(-1, 1) from Philox keyed (seed, env,
    episode) under the Pendulum key - the engine's own stream, as for CartPole (not gymnasium's np_random)."""
    x, y, _, _ = px.philox4x32_10(seed, env.astype(np.uint32), 0x9E4D0000, episode.astype(np.uint32), 0)
    return np.stack([_fma32(px.u01(x), PEND_2PI, -PEND_PI), _fma32(px.u01(y), np.float32(2.0), np.float32(-1.0))],
                    axis=-1).astype(np.float32)


class PendulumEnvOracle:
    """Vectorised Pendulum-v1 on the host with the device env's semantics (csrc/orl_env.h): pendulum_step_f32, no
    termination, truncation at ``episode_limit`` = 200 with ``done`` and auto-reset to the Philox start state of
    (seed, env, episode) - the observation of the NEW episode returned.  Duck-typed like CartPoleEnvOracle."""

    def __init__(self, n_envs, seed, episode_limit=200):
        self.N, self.seed, self.limit = n_envs, seed, episode_limit
        self.reset()

    def reset(self):
        self.episode = np.zeros(self.N, np.int64)
        self.steps = np.zeros(self.N, np.int64)
        self.state = pendulum_reset_state(self.seed, np.arange(self.N), self.episode)
        return pendulum_obs_f32(self.state)[:, None, :]

    def step(self, actions):
        a = np.asarray(actions, np.float32).reshape(self.N)
        nxt, obs, rew = pendulum_step_f32(self.state, a)
        self.steps = self.steps + 1
        done = self.steps >= self.limit
        self.episode = np.where(done, self.episode + 1, self.episode)
        fresh = pendulum_reset_state(self.seed, np.arange(self.N), self.episode)
        self.state = np.where(done[:, None], fresh, nxt).astype(np.float32)
        obs = np.where(done[:, None], pendulum_obs_f32(fresh), obs).astype(np.float32)
        self.steps = np.where(done, 0, self.steps)
        return obs[:, None, :], rew.reshape(self.N, 1, 1), done[:, None], [{} for _ in range(self.N)]


class GaussianCPUTrainer(CPUTrainer):
    """CPUTrainer with a Box(n_actions) action space (DiagGaussian head, no action masks) and discount ``gamma`` /
    ``gae_lambda``.  Same construction order - seeds, policy tower, critic tower, Adam states, env reset - so the random
    streams are consumed the way CPUTrainer consumes them."""

    def __init__(self, n_envs: int, T: int, env, obs_dim: int = 3, n_actions: int = 1, seed: int = 0, ppo_epoch: int = 10,
                 num_mini_batch: int = 1, hp: po.PPOHyper = None, lr: float = 5e-4, threads: int = None,
                 gamma: float = 0.99, gae_lambda: float = 0.95):
        if threads:
            torch.set_num_threads(threads)
        self.N, self.T, self.D, self.K = n_envs, T, obs_dim, n_actions
        self.hp = hp or po.PPOHyper()
        self.ppo_epoch, self.nmb = ppo_epoch, num_mini_batch
        self.gamma, self.gae_lambda = gamma, gae_lambda
        import random

        random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
        self.pspec = po.TowerSpec(obs_dim, n_actions, po.HEAD_GAUSSIAN)
        self.cspec = po.TowerSpec(obs_dim, 1, po.HEAD_VALUE)
        self.ptheta = po.init_tower(self.pspec, 0.01)
        self.ctheta = po.init_tower(self.cspec, 1.0)
        self.padam = po.AdamOracle(self.ptheta.numel(), lr)
        self.cadam = po.AdamOracle(self.ctheta.numel(), lr)
        self.vn = po.ValueNormOracle() if self.hp.use_valuenorm else None
        self.env = env
        self.buf = CPUReplayData(T, n_envs, 1, obs_dim, n_actions, 0)
        self.buf.policy_obs[0] = self.env.reset()
        self.buf.critic_obs[0] = self.buf.policy_obs[0]
        self.phase = {"act": 0.0, "env": 0.0, "insert": 0.0, "gae": 0.0, "update": 0.0}

    @torch.no_grad()
    def _act(self, step):  # onpolicy_driver.py:235-279 with the DiagGaussian head of ACTLayer
        b, N = self.buf, self.N
        cobs, pobs = b.get_batch_data("critic_obs", step), b.get_batch_data("policy_obs", step)
        rnn, rnn_c = b.get_batch_data("rnn_states", step), b.get_batch_data("rnn_states_critic", step)
        b.get_batch_data("masks", step)
        mean = po.tower_forward(self.pspec, self.ptheta, torch.from_numpy(pobs))
        std = self.pspec.split(self.ptheta)["logstd"].exp()
        dist = torch.distributions.Normal(mean, std.expand_as(mean))
        action = dist.sample()
        # per-dimension log-probs, the buffer layout po.evaluate_actions reads (= the summed log-prob for Box(1))
        logp = dist.log_prob(action)
        value = po.tower_forward(self.cspec, self.ctheta, torch.from_numpy(cobs))
        sp = lambda x: np.array(np.split(x, N))
        return (sp(value.numpy()), sp(action.numpy()), sp(logp.numpy()), sp(rnn), sp(rnn_c))

    def update(self) -> Dict[str, float]:  # CPUTrainer.update with gamma / gae_lambda
        b = self.buf
        t0 = time.perf_counter()
        with torch.no_grad():  # compute_returns (onpolicy_driver.py:205-233)
            nv = po.tower_forward(self.cspec, self.ctheta, torch.from_numpy(b.get_batch_data("critic_obs", -1)))
        next_values = np.array(np.split(nv.numpy(), self.N))
        vn = self.vn if self.hp.use_valuenorm else None
        b.returns, b.value_preds = po.compute_returns(b.rewards, b.value_preds, b.masks, b.bad_masks, next_values,
                                                      self.gamma, self.gae_lambda, True, False, vn)
        t1 = time.perf_counter()
        bufd = dict(critic_obs=b.critic_obs, policy_obs=b.policy_obs, actions=b.actions, value_preds=b.value_preds,
                    returns=b.returns, active_masks=b.active_masks, action_log_probs=b.action_log_probs,
                    action_masks=None)
        info, _, _ = po.train_ppo(self.hp, self.pspec, self.ptheta, self.cspec, self.ctheta, self.padam, self.cadam, vn,
                                  bufd, self.ppo_epoch, self.nmb)
        b.after_update()
        t2 = time.perf_counter()
        self.phase["gae"] += t1 - t0
        self.phase["update"] += t2 - t1
        return info
