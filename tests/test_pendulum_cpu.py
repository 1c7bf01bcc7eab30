"""Pendulum-v1 (device env ORL_ENV_PENDULUM) without a GPU: the fp32 restatement of csrc/orl_env.h
(tests/pendulum_oracle.py pendulum_step_f32) against a float64 transcription of gymnasium's step (classic_control/pendulum.py), the ABI constant and
argument checks, make()'s refusal without a GPU, and one CPU-port iteration with the Gaussian head."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from oracle import ppo_oracle as po
from tests import pendulum_oracle as pend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (th, thdot, action): torque clip, speed clip, th either side of +-pi, negative arguments of angle_normalize
CASES = [
    (0.3, 0.5, 5.0),        # |a| > 2: the torque clips to +2
    (-1.2, -0.7, -3.5),     # ... and to -2 (angle_normalize of a negative angle)
    (2.0, 7.9, 2.0),        # newthdot above 8: the speed clips
    (-2.0, -7.95, -2.0),    # newthdot below -8
    (3.1, 1.0, 0.0),        # th just below pi: the new angle crosses pi (wrapped to the other side)
    (-3.1, -1.0, 0.0),      # th just above -pi, crossing -pi
    (3.14159, 0.2, 0.1),    # th a hair below pi
    (-3.14159, -0.2, -0.1),
    (-0.01, -0.02, 0.5),    # small negative th: the argument of the modulo is positive, a negative thdot
    (-2.5, 3.0, -1.0),      # fmod's sign: x + pi > 0 yet th < 0
    (0.0, 0.0, 0.0),
    (1.5707964, -4.0, 1.999),
]


def _f64_obs(th, thdot):
    return np.array([math.cos(th), math.sin(th), thdot])


@pytest.mark.parametrize("th,thdot,a", CASES)
def test_fp32_restatement_matches_the_float64_gymnasium_step(th, thdot, a):
    st = np.array([[th, thdot]], np.float32)
    nxt, obs, r = pend.pendulum_step_f32(st, np.array([a], np.float32))
    # the inputs themselves are float32 roundings of the case: transcribe from those
    th32, thdot32 = float(st[0, 0]), float(st[0, 1])
    nth64, ndot64, r64 = pend.pendulum_step_f64(th32, thdot32, np.float32(a))
    np.testing.assert_allclose(obs[0], _f64_obs(nth64, ndot64), rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(r[0], r64, rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(nxt[0, 1], ndot64, rtol=2e-6, atol=2e-6)
    # the wrapped fp32 angle is the float64 one modulo 2 pi, inside [-pi, pi)
    d = (float(nxt[0, 0]) - nth64 + math.pi) % (2 * math.pi) - math.pi
    assert abs(d) < 4e-6, (nxt[0, 0], nth64)
    assert -math.pi - 1e-6 <= nxt[0, 0] < math.pi + 1e-6


def test_clips_and_angle_normalize_sign():
    f = np.float32
    # torque clip: a = 5 costs like a = 2; speed clip: |newthdot| <= 8
    _, _, r5 = pend.pendulum_step_f32(np.array([[0.3, 0.5]], f), np.array([5.0], f))
    _, _, r2 = pend.pendulum_step_f32(np.array([[0.3, 0.5]], f), np.array([2.0], f))
    assert r5[0] == r2[0]
    nxt, _, _ = pend.pendulum_step_f32(np.array([[2.0, 7.9], [-2.0, -7.95]], f), np.array([2.0, -2.0], f))
    assert nxt[0, 1] == 8.0 and nxt[1, 1] == -8.0
    # floored modulo: for x + pi < 0 a truncating fmod without the sign fix would return a value 2 pi too low
    x = np.array([-3.0, -4.0, -7.0, 4.0, 10.0, -10.0], f)
    want = ((x.astype(np.float64) + np.pi) % (2 * np.pi)) - np.pi
    np.testing.assert_allclose(pend.pendulum_angle_normalize_f32(x), want, rtol=0, atol=2e-6)


def test_reset_states_are_in_range_and_keyed_by_episode():
    s0 = pend.pendulum_reset_state(5, np.arange(1000), np.zeros(1000))
    s1 = pend.pendulum_reset_state(5, np.arange(1000), np.ones(1000))
    assert s0.dtype == np.float32 and s0.shape == (1000, 2)
    assert np.all(s0[:, 0] >= -np.pi - 1e-6) and np.all(s0[:, 0] < np.pi + 1e-6)
    assert np.all(np.abs(s0[:, 1]) <= 1.0)
    assert not np.array_equal(s0, s1)


def test_oracle_env_truncates_at_200_and_auto_resets():
    env = pend.PendulumEnvOracle(5, 3)
    obs = env.reset()
    assert obs.shape == (5, 1, 3)
    for t in range(1, 401):
        obs, r, d, _ = env.step(np.full((5, 1, 1), 0.5, np.float32))
        assert r.shape == (5, 1, 1) and np.all(r <= 0)
        assert d.shape == (5, 1) and bool(d.all()) == (t % 200 == 0) and bool(d.any()) == (t % 200 == 0)
    want = pend.pendulum_obs_f32(pend.pendulum_reset_state(3, np.arange(5), np.full(5, 2)))
    np.testing.assert_array_equal(obs[:, 0], want)


def test_header_constant_equals_native():
    from openrl_amd import _native as n

    text = open(os.path.join(ROOT, "include", "orl_hip.h")).read()
    m = re.search(r"#define ORL_ENV_PENDULUM (\d+)", text)
    assert m and int(m.group(1)) == n.ORL_ENV_PENDULUM == 5
    assert n.ORL_VERSION == 306


def test_state_width_and_fused_rollout_argument_checks():
    """Pendulum's fused rollout takes a Gaussian head with n_out 1 and 3-d obs, on the chain kernel only: every other
    request returns ORL_E_INVALID with a message before anything is launched."""
    from openrl_amd import _native as n

    lib = n.load()
    assert lib.orl_env_state_width(n.ORL_ENV_PENDULUM) == 4
    fake = 4096  # non-null placeholders: validation fails before any pointer is used
    buf = n.BufferPtrs()
    for f in ("policy_obs", "critic_obs", "rewards", "masks", "bad_masks", "active_masks"):
        setattr(buf, f, fake)
    buf.T, buf.N, buf.A, buf.Dp, buf.Dc = 8, 16, 1, 3, 3
    args = n.RolloutArgs(buf, fake, fake, fake, fake, fake, n.ORL_ENV_PENDULUM, 200, 1, 2, 0)
    cri = n.NetDesc(3, 64, 1, n.ORL_HEAD_VALUE)
    for pol in (n.NetDesc(3, 64, 2, n.ORL_HEAD_CATEGORICAL), n.NetDesc(3, 64, 2, n.ORL_HEAD_GAUSSIAN)):
        rc = lib.orl_rollout_fused(C.byref(pol), C.c_void_p(fake), C.byref(cri), C.c_void_p(fake), C.byref(args), None, None)
        assert rc == -1 and b"Pendulum" in lib.orl_last_error_string()
    pol = n.NetDesc(3, 64, 1, n.ORL_HEAD_GAUSSIAN)
    args.opp_reserved = 1
    rc = lib.orl_rollout_fused(C.byref(pol), C.c_void_p(fake), C.byref(cri), C.c_void_p(fake), C.byref(args), None, None)
    assert rc == -1 and b"lockstep" in lib.orl_last_error_string()


def test_make_pendulum_needs_a_gpu():
    from openrl_amd import _native as nat
    from openrl_amd.envs.common import make

    with pytest.raises(nat.NativeError):
        make("Pendulum-v1", env_num=2, seed=0)


def test_cpu_port_gaussian_iteration_on_the_pendulum_oracle():
    N, T = 8, 16
    tr = pend.GaussianCPUTrainer(N, T, pend.PendulumEnvOracle(N, 0), obs_dim=3, n_actions=1, seed=0, ppo_epoch=2,
                                 threads=2)
    th0 = tr.ptheta.clone()
    tr.rollout()
    b = tr.buf
    assert b.actions.shape == (T, N, 1, 1) and b.action_log_probs.shape == (T, N, 1, 1) and b.action_masks is None
    assert np.all(np.isfinite(b.actions)) and np.all(b.rewards <= 0)
    # the stored log-prob is Normal(mean, exp(logstd)).log_prob of the stored (unclipped) action
    _, mean, _ = po.get_actions(tr.pspec, th0, tr.cspec, tr.ctheta, b.policy_obs[0, :, 0], b.policy_obs[0, :, 0], None,
                                True)
    std = float(np.exp(tr.pspec.split(th0)["logstd"].numpy()[0]))
    a = b.actions[0, :, 0, 0]
    lp = -((a - mean[:, 0]) ** 2) / (2 * std * std) - math.log(std) - 0.5 * math.log(2 * math.pi)
    np.testing.assert_allclose(b.action_log_probs[0, :, 0, 0], lp, rtol=1e-4, atol=1e-5)
    info = tr.update()
    assert np.isfinite(info["value_loss"]) and np.isfinite(info["policy_loss"])
    assert not np.array_equal(th0.numpy(), tr.ptheta.numpy())
