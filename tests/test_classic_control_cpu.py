"""Acrobot-v1 and MountainCar-v0 (device envs ORL_ENV_ACROBOT / ORL_ENV_MOUNTAINCAR) without a GPU: the fp32
restatements of csrc/orl_env.h (tests/classic_control_oracle.py) against float64 transcriptions of gymnasium's steps, the
reset streams, the oracle envs' truncation and auto-reset, the ABI constants and argument checks, make()'s refusal
without a GPU, and one CPU-port iteration on each oracle env."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import classic_control_oracle as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = math.pi


@pytest.fixture(autouse=True)
def _leave_the_global_rngs_as_found():
    """The CPU port seeds the process-wide generators (random, numpy, torch) and sets torch's thread count; later tests
    in the same process draw their initial weights from them (orthogonal initialisation's QR rounds differently with
    other thread counts), so every test here leaves them as it found them."""
    import random

    import torch

    threads = torch.get_num_threads()
    state = (random.getstate(), np.random.get_state(), torch.get_rng_state())
    yield
    random.setstate(state[0]); np.random.set_state(state[1]); torch.set_rng_state(state[2])
    torch.set_num_threads(threads)


# (th1, th2, dth1, dth2): rest, small swings, the wrap edges (angles next to +-pi, fast enough to cross), the speed bounds,
# and the terminal boundary -cos th1 - cos(th1 + th2) = 1 from both sides
ACRO_STATES = [
    (0.0, 0.0, 0.0, 0.0),
    (0.05, -0.08, 0.09, -0.02),
    (3.1, 0.2, 3.0, 1.0),                # th1 crosses +pi during the step: wrapped to the other side
    (-3.1, -0.3, -3.0, -2.0),            # ... and -pi
    (0.4, 3.13, 0.5, 5.0),               # th2 crosses +pi
    (1.0, -3.13, -0.2, -6.0),            # th2 crosses -pi
    (0.3, 0.1, 4.0 * PI - 0.01, 1.0),    # dth1 at its bound
    (-0.3, 0.1, -4.0 * PI + 0.01, -9.0 * PI + 0.02),  # both speeds at their bounds
    (0.2, -0.1, 1.0, 9.0 * PI - 0.05),
    (2.0, 0.0, 0.0, 0.0),                # -cos th1 - cos(th1 + th2) = 2 * 0.416 < 1: just short of terminal
    (2.1, 0.0, 0.3, 0.0),                # ... and beyond it: 2 * 0.505 > 1
    (2.094, 0.0, 0.0, 0.0),              # th1 ~ 2 pi / 3: on the boundary
    (PI, 0.0, 0.0, 0.0),                 # upright
    (-2.5, 1.0, -1.5, 2.5),
]
MCAR_STATES = [
    (-0.5, 0.0),
    (-1.19, -0.02),   # the left wall: position clips to -1.2, a negative velocity drops to 0
    (-1.2, -0.001),
    (-1.2, 0.0),
    (0.5, 0.0),       # at the goal with v = 0 (action 1 / 2 keeps v >= 0 there)
    (0.5, -0.001),    # at the goal with v < 0
    (0.49, 0.0105),   # reaches the goal in this step
    (0.59, 0.07),     # the right bound: position clips to 0.6
    (0.0, 0.0699),    # velocity clips to +0.07
    (-0.3, -0.0699),  # ... and to -0.07
]


def _acro_obs64(s):
    return np.array([math.cos(s[0]), math.sin(s[0]), math.cos(s[1]), math.sin(s[1]), s[2], s[3]])


def _angle_diff(a, b):
    return (a - b + PI) % (2 * PI) - PI


@pytest.mark.parametrize("state", ACRO_STATES)
@pytest.mark.parametrize("action", [0, 1, 2])
def test_acrobot_fp32_step_matches_the_float64_gymnasium_step(state, action):
    st = np.array([state], np.float32)
    nxt, obs, term, rew = cc.acrobot_step_f32(st, np.array([action]))
    ns64, term64, r64 = cc.acrobot_step_f64(st[0].astype(np.float64), action)
    # angles: the same point on the circle (a value next to +-pi may land on either side in fp32), inside [-pi, pi]
    for k in range(2):
        assert abs(_angle_diff(float(nxt[0, k]), ns64[k])) < 2e-5, (k, nxt[0], ns64)
        assert -PI - 1e-6 <= nxt[0, k] <= PI + 1e-6
    np.testing.assert_allclose(nxt[0, 2:], ns64[2:], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(obs[0], _acro_obs64(ns64), rtol=2e-5, atol=2e-5)
    # the terminal test agrees unless the float64 state lies within rounding of the boundary
    margin = -math.cos(ns64[0]) - math.cos(ns64[1] + ns64[0]) - 1.0
    if abs(margin) > 1e-4:
        assert bool(term[0]) == term64 and rew[0] == r64
    assert rew[0] == (0.0 if term[0] else -1.0)


def test_acrobot_bounds_and_wrap_edges():
    f = np.float32
    x = np.array([PI + 0.01, -PI - 0.01, 3 * PI + 0.1, -5 * PI - 0.1, PI, -PI, 0.5], f)
    w = cc.acrobot_wrap_f32(x)
    assert np.all(w <= np.float32(PI)) and np.all(w >= -np.float32(PI))
    np.testing.assert_allclose(_angle_diff(w.astype(np.float64), x.astype(np.float64)), 0.0, atol=3e-6)
    assert w[4] == x[4] and w[5] == x[5] and w[6] == x[6]  # gymnasium's wrap leaves +-pi themselves alone
    # a huge torque-free fall: the speeds stay inside +-4 pi / +-9 pi
    s = np.array([[0.0, 0.0, 4 * PI, 9 * PI], [0.0, 0.0, -4 * PI, -9 * PI]], f)
    nxt, _, _, _ = cc.acrobot_step_f32(s, np.array([2, 0]))
    assert np.all(np.abs(nxt[:, 2]) <= f(4 * PI)) and np.all(np.abs(nxt[:, 3]) <= f(9 * PI))


@pytest.mark.parametrize("state", MCAR_STATES)
@pytest.mark.parametrize("action", [0, 1, 2])
def test_mountaincar_fp32_step_matches_the_float64_gymnasium_step(state, action):
    st = np.array([state], np.float32)
    nxt, term, rew = cc.mountaincar_step_f32(st, np.array([action]))
    ns64, term64, r64 = cc.mountaincar_step_f64(st[0].astype(np.float64), action)
    np.testing.assert_allclose(nxt[0], ns64, rtol=0, atol=2e-7)
    assert rew[0] == r64 == -1.0
    if abs(ns64[0] - 0.5) > 1e-6 or ns64[1] != 0.0:
        assert bool(term[0]) == term64


def test_mountaincar_left_wall_and_goal_edges():
    f = np.float32
    nxt, term, _ = cc.mountaincar_step_f32(np.array([[-1.19, -0.02], [-1.2, 0.0]], f), np.array([0, 0]))
    assert nxt[0, 0] == f(-1.2) and nxt[0, 1] == 0.0 and not term.any()
    # p = 0.5 with v = 0: pushing right keeps v >= 0 and the episode ends; with v < 0 and no push it does not
    nxt, term, _ = cc.mountaincar_step_f32(np.array([[0.5, 0.0], [0.5, -0.001]], f), np.array([2, 1]))
    assert term[0] and nxt[0, 0] >= 0.5 and not term[1]


def test_reset_ranges_and_keyed_by_episode():
    env = np.arange(2000)
    a0, a1 = cc.acrobot_reset_state(7, env, np.zeros(2000)), cc.acrobot_reset_state(7, env, np.ones(2000))
    assert a0.dtype == np.float32 and a0.shape == (2000, 4)
    assert np.all(np.abs(a0) <= 0.1) and a0.min() < -0.09 and a0.max() > 0.09
    assert not np.array_equal(a0, a1)
    np.testing.assert_array_equal(a0, cc.acrobot_reset_state(7, env, np.zeros(2000)))
    m0, m1 = cc.mountaincar_reset_state(7, env, np.zeros(2000)), cc.mountaincar_reset_state(7, env, np.ones(2000))
    assert m0.shape == (2000, 2) and np.all(m0[:, 1] == 0.0)
    assert np.all(m0[:, 0] >= -0.6) and np.all(m0[:, 0] <= -0.4) and m0[:, 0].min() < -0.59 and m0[:, 0].max() > -0.41
    assert not np.array_equal(m0, m1)
    assert not np.array_equal(cc.acrobot_reset_state(8, env, np.zeros(2000)), a0)


def test_oracle_envs_truncate_and_auto_reset():
    # MountainCar with no push never reaches the goal: done exactly at 200 and 400, the observation of episode 2
    env = cc.MountainCarEnvOracle(5, 3)
    assert env.reset().shape == (5, 1, 2)
    for t in range(1, 401):
        obs, r, d, _ = env.step(np.ones((5, 1, 1)))
        assert r.shape == (5, 1, 1) and np.all(r == -1.0)
        assert bool(d.all()) == (t % 200 == 0) and bool(d.any()) == (t % 200 == 0)
    np.testing.assert_array_equal(obs[:, 0], cc.mountaincar_reset_state(3, np.arange(5), np.full(5, 2)))
    # Acrobot under zero torque from a small start state swings but never terminates within 500 steps
    env = cc.AcrobotEnvOracle(4, 1)
    assert env.reset().shape == (4, 1, 6)
    for t in range(1, 501):
        obs, r, d, _ = env.step(np.ones((4, 1, 1)))
        assert np.all(r == -1.0) and bool(d.any()) == (t == 500)
    want = cc.acrobot_obs_f32(cc.acrobot_reset_state(1, np.arange(4), np.ones(4)))
    np.testing.assert_array_equal(obs[:, 0], want)
    # a terminal step: reward 0, done, the reset observation of the next episode
    env = cc.AcrobotEnvOracle(1, 2)
    env.state = np.array([[2.5, 0.0, 0.0, 0.0]], np.float32)
    obs, r, d, _ = env.step(np.ones((1, 1, 1)))
    assert r[0, 0, 0] == 0.0 and d[0, 0] and env.episode[0] == 1 and env.steps[0] == 0
    np.testing.assert_array_equal(obs[:, 0], cc.acrobot_obs_f32(cc.acrobot_reset_state(2, np.arange(1), np.ones(1))))


def test_header_constants_equal_native():
    from openrl_amd import _native as n
    from openrl_amd import ops

    text = open(os.path.join(ROOT, "include", "orl_hip.h")).read()
    for name, v in (("ORL_ENV_ACROBOT", 6), ("ORL_ENV_MOUNTAINCAR", 7)):
        m = re.search(r"#define %s (\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(n, name) == v
    assert (ops.ENV_ACROBOT, ops.ENV_MOUNTAINCAR) == (6, 7)
    assert n.ORL_VERSION == 306
    env_h = open(os.path.join(ROOT, "openrl_amd", "csrc", "orl_env.h")).read()
    assert re.search(r"ACROBOT_STATE_W = %d;" % cc.ACROBOT_STATE_W, env_h)
    assert re.search(r"MOUNTAINCAR_STATE_W = %d;" % cc.MOUNTAINCAR_STATE_W, env_h)
    assert "0x%Xu" % cc.ACROBOT_KEY in env_h and "0x%Xu" % cc.MOUNTAINCAR_KEY in env_h


@pytest.mark.parametrize("kind,name,D,width", [("ORL_ENV_ACROBOT", b"Acrobot", 6, 6),
                                              ("ORL_ENV_MOUNTAINCAR", b"MountainCar", 2, 4)])
def test_state_width_and_fused_rollout_argument_checks(kind, name, D, width):
    """The fused rollout takes Discrete(3) with the env's observation width, on the chain kernel only: every other
    request returns ORL_E_INVALID with a message before anything is launched."""
    from openrl_amd import _native as n

    lib = n.load()
    env_kind = getattr(n, kind)
    assert lib.orl_env_state_width(env_kind) == width
    fake = 4096  # non-null placeholders: validation fails before any pointer is used
    buf = n.BufferPtrs()
    for f in ("policy_obs", "critic_obs", "rewards", "masks", "bad_masks", "active_masks"):
        setattr(buf, f, fake)
    buf.T, buf.N, buf.A, buf.Dp, buf.Dc = 8, 16, 1, D, D
    args = n.RolloutArgs(buf, fake, fake, fake, fake, fake, env_kind, 200, 1, 2, 0)
    cri = n.NetDesc(D, 64, 1, n.ORL_HEAD_VALUE)
    for pol in (n.NetDesc(D, 64, 2, n.ORL_HEAD_CATEGORICAL), n.NetDesc(D, 64, 4, n.ORL_HEAD_CATEGORICAL),
                n.NetDesc(D, 64, 3, n.ORL_HEAD_GAUSSIAN)):
        rc = lib.orl_rollout_fused(C.byref(pol), C.c_void_p(fake), C.byref(cri), C.c_void_p(fake), C.byref(args), None, None)
        assert rc == -1 and name in lib.orl_last_error_string()
    # the wrong observation width
    buf.Dp = buf.Dc = D + 1
    args = n.RolloutArgs(buf, fake, fake, fake, fake, fake, env_kind, 200, 1, 2, 0)
    pol, cri2 = n.NetDesc(D + 1, 64, 3, n.ORL_HEAD_CATEGORICAL), n.NetDesc(D + 1, 64, 1, n.ORL_HEAD_VALUE)
    rc = lib.orl_rollout_fused(C.byref(pol), C.c_void_p(fake), C.byref(cri2), C.c_void_p(fake), C.byref(args), None, None)
    assert rc == -1 and name in lib.orl_last_error_string()
    buf.Dp = buf.Dc = D
    args = n.RolloutArgs(buf, fake, fake, fake, fake, fake, env_kind, 200, 1, 2, 0)
    pol = n.NetDesc(D, 64, 3, n.ORL_HEAD_CATEGORICAL)
    args.opp_reserved = 1
    rc = lib.orl_rollout_fused(C.byref(pol), C.c_void_p(fake), C.byref(cri), C.c_void_p(fake), C.byref(args), None, None)
    assert rc == -1 and b"lockstep" in lib.orl_last_error_string()


@pytest.mark.parametrize("env_id", ["Acrobot-v1", "MountainCar-v0"])
def test_make_needs_a_gpu(env_id):
    from openrl_amd import _native as nat
    from openrl_amd.envs.common import make

    with pytest.raises(nat.NativeError):
        make(env_id, env_num=2, seed=0)


@pytest.mark.parametrize("which", ["acrobot", "mountaincar"])
def test_cpu_port_iteration_on_the_oracle_env(which):
    from oracle.cpu_trainer import CPUTrainer

    N, T = 8, 16
    env, D = (cc.AcrobotEnvOracle(N, 0), 6) if which == "acrobot" else (cc.MountainCarEnvOracle(N, 0), 2)
    tr = CPUTrainer(N, T, obs_dim=D, n_actions=3, seed=0, ppo_epoch=2, threads=2, env=env)
    th0 = tr.ptheta.clone()
    tr.rollout()
    b = tr.buf
    assert b.policy_obs.shape == (T + 1, N, 1, D) and b.actions.shape == (T, N, 1, 1)
    assert set(np.unique(b.actions).tolist()) <= {0.0, 1.0, 2.0}
    assert np.all(b.rewards == -1.0)
    info = tr.update()
    assert np.isfinite(info["policy_loss"]) and not np.array_equal(th0.numpy(), tr.ptheta.numpy())
