"""MountainCarContinuous-v0 (device env ORL_ENV_MOUNTAINCAR_CONT) without a GPU: the fp32 restatement of csrc/orl_env.h
(tests/mountaincar_continuous_oracle.py) against the float64 transcription of gymnasium's step, its edges (the left wall,
the goal, the force clip that the reward does not see, the speed clamp), the reset stream, the oracle env's termination,
truncation and auto-reset, the ABI constants and argument checks, make()'s refusal without a GPU, and one CPU-port
iteration on the oracle env."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import mountaincar_continuous_oracle as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(autouse=True)
def _leave_the_global_rngs_as_found():
    """The CPU port seeds the process-wide generators (random, numpy, torch) and sets torch's thread count; later tests
    in the same process draw their initial weights from them, so every test here leaves them as it found them."""
    import random

    import torch

    threads = torch.get_num_threads()
    state = (random.getstate(), np.random.get_state(), torch.get_rng_state())
    yield
    random.setstate(state[0]); np.random.set_state(state[1]); torch.set_rng_state(state[2])
    torch.set_num_threads(threads)


def _check_against_f64(states, actions):
    """Every row: next state within 2e-7 (a few float32 ulps of the position), reward within 1e-5 relative, the
    terminal flag equal unless the float64 state lies within rounding of the goal."""
    nxt, term, rew = mc.mountaincar_cont_step_f32(states, actions)
    n_term = 0
    for i in range(len(states)):
        ns64, term64, r64 = mc.mountaincar_cont_step_f64(states[i].astype(np.float64), float(actions[i]))
        np.testing.assert_allclose(nxt[i], ns64, rtol=0, atol=2e-7, err_msg=str((states[i], actions[i])))
        edge = abs(float(ns64[0]) - 0.45) < 1e-6 or abs(float(ns64[1])) < 1e-9
        if not edge:
            assert bool(term[i]) == term64, (states[i], actions[i])
            np.testing.assert_allclose(rew[i], r64, rtol=1e-5, atol=1e-7)
        n_term += int(term[i])
    return n_term


def test_fp32_step_matches_the_float64_gymnasium_step_on_random_states():
    rs = np.random.RandomState(0)
    n = 4000
    states = np.stack([rs.uniform(-1.2, 0.6, n), rs.uniform(-0.07, 0.07, n)], axis=-1).astype(f32)
    actions = rs.uniform(-2.5, 2.5, n).astype(f32)
    n_term = _check_against_f64(states, actions)
    assert n_term > 50  # the right part of the hill reaches the goal from many of these states


def test_left_wall_with_negative_velocity():
    # (gravity pushes right at the wall, +0.0022 per step: these velocities still carry the car into it)
    st = np.array([[-1.19, -0.02], [-1.2, -0.01], [-1.18, -0.03], [-1.15, -0.07]], f32)
    a = np.array([-1.0, -0.3, -1.0, -4.0], f32)
    nxt, term, rew = mc.mountaincar_cont_step_f32(st, a)
    assert np.all(nxt[:, 0] == f32(-1.2)) and np.all(nxt[:, 1] == 0.0) and not term.any()
    _check_against_f64(st, a)
    # rising off the wall: the velocity is kept
    nxt, _, _ = mc.mountaincar_cont_step_f32(np.array([[-1.2, 0.0]], f32), np.array([1.0], f32))
    assert nxt[0, 0] > f32(-1.2) and nxt[0, 1] > 0


def test_exactly_at_the_goal():
    """The goal is inclusive in both coordinates: landing on p = 0.45 with v = 0 exactly terminates, the next float below
    either does not.  v lands on exactly 0 when it starts at minus the step's increment."""
    p = np.array([0.45, 0.45, np.nextafter(f32(0.45), f32(-1))], f32)
    force = np.array([0.5, 0.5, 0.5], f32)
    inc = mc._fma32(force, mc.POWER, mc.mountaincar_pre_f32(p))
    v0 = (-inc).astype(f32)
    v0[1] = np.nextafter(v0[1], f32(-1))  # lands on the largest negative float below 0
    st = np.stack([p, v0], axis=-1).astype(f32)
    nxt, term, rew = mc.mountaincar_cont_step_f32(st, force)
    assert nxt[0, 0] == f32(0.45) and nxt[0, 1] == 0.0 and term[0]
    assert nxt[1, 1] < 0 and not term[1]
    assert nxt[2, 0] < f32(0.45) and nxt[2, 1] == 0.0 and not term[2]
    assert rew[0] == f32(100.0) - f32(f32(0.25) * f32(0.1)) and rew[1] == -f32(f32(0.25) * f32(0.1))
    # the goal is 0.45, not MountainCar-v0's 0.5
    nxt, term, _ = mc.mountaincar_cont_step_f32(np.array([[0.46, 0.0], [0.41, 0.045]], f32), np.array([1.0, 1.0], f32))
    assert term[0] and nxt[0, 0] < 0.5 and term[1] and nxt[1, 0] < 0.5


def test_force_is_clipped_but_the_reward_is_not():
    st = np.repeat(np.array([[-0.5, 0.01]], f32), 6, axis=0)
    a = np.array([1.0, 3.0, 17.5, -1.0, -3.0, -17.5], f32)
    nxt, term, rew = mc.mountaincar_cont_step_f32(st, a)
    np.testing.assert_array_equal(nxt[1], nxt[0]); np.testing.assert_array_equal(nxt[2], nxt[0])
    np.testing.assert_array_equal(nxt[4], nxt[3]); np.testing.assert_array_equal(nxt[5], nxt[3])
    assert not term.any()
    want = -((a * a).astype(f32) * f32(0.1)).astype(f32)
    np.testing.assert_array_equal(rew, want)
    np.testing.assert_allclose(rew, [-0.1, -0.9, -30.625, -0.1, -0.9, -30.625], rtol=1e-6)
    _check_against_f64(st, a)


def test_speed_clamp():
    # (where the slope pulls the same way as the force: cos(3 p) < 0 for v > 0, > 0 for v < 0)
    st = np.array([[-0.8, 0.0699], [-0.3, -0.0699], [-0.7, 0.07], [0.0, -0.07]], f32)
    a = np.array([1.0, -1.0, 5.0, -5.0], f32)
    nxt, _, _ = mc.mountaincar_cont_step_f32(st, a)
    np.testing.assert_array_equal(np.abs(nxt[:, 1]), np.full(4, f32(0.07)))
    assert np.all(np.sign(nxt[:, 1]) == np.sign(st[:, 1]))
    _check_against_f64(st, a)


def test_reset_stream_range_and_independence():
    env = np.arange(2000)
    m0 = mc.mountaincar_cont_reset_state(7, env, np.zeros(2000))
    m1 = mc.mountaincar_cont_reset_state(7, env, np.ones(2000))
    assert m0.dtype == np.float32 and m0.shape == (2000, 2) and np.all(m0[:, 1] == 0.0)
    for m in (m0, m1):
        assert np.all(m[:, 0] >= -0.6) and np.all(m[:, 0] <= -0.4) and m[:, 0].min() < -0.59 and m[:, 0].max() > -0.41
    # independent across episodes and envs: no repeats, and no correlation between consecutive episodes or envs
    assert len(np.unique(np.concatenate([m0[:, 0], m1[:, 0]]))) > 3990
    assert abs(np.corrcoef(m0[:, 0], m1[:, 0])[0, 1]) < 0.1
    assert abs(np.corrcoef(m0[:-1, 0], m0[1:, 0])[0, 1]) < 0.1
    np.testing.assert_array_equal(m0, mc.mountaincar_cont_reset_state(7, env, np.zeros(2000)))
    assert not np.array_equal(mc.mountaincar_cont_reset_state(8, env, np.zeros(2000)), m0)
    # not MountainCar-v0's stream
    from tests import classic_control_oracle as cc

    assert not np.array_equal(cc.mountaincar_reset_state(7, env, np.zeros(2000)), m0)


def test_oracle_env_terminates_truncates_and_auto_resets():
    # no force never reaches the goal: done exactly at 999 and 1998, reward 0 on every step
    env = mc.MountainCarContinuousEnvOracle(5, 3)
    assert env.reset().shape == (5, 1, 2)
    for t in range(1, 2 * 999 + 1):
        obs, r, d, _ = env.step(np.zeros((5, 1, 1), f32))
        assert r.shape == (5, 1, 1) and np.all(r == 0.0)
        assert bool(d.all()) == (t % 999 == 0) and bool(d.any()) == (t % 999 == 0)
    np.testing.assert_array_equal(obs[:, 0], mc.mountaincar_cont_reset_state(3, np.arange(5), np.full(5, 2)))
    # a short limit truncates first
    env = mc.MountainCarContinuousEnvOracle(2, 1, episode_limit=7)
    for t in range(1, 8):
        _, _, d, _ = env.step(np.ones((2, 1, 1), f32))
    assert d.all() and np.all(env.episode == 1)
    # a terminal step: reward 100 - 0.1 a^2, done, the reset observation of the next episode
    env = mc.MountainCarContinuousEnvOracle(1, 2)
    env.state = np.array([[0.44, 0.02]], f32)
    obs, r, d, _ = env.step(np.full((1, 1, 1), 2.0, f32))
    assert r[0, 0, 0] == f32(100.0) - f32(0.4) and d[0, 0] and env.episode[0] == 1 and env.steps[0] == 0
    np.testing.assert_array_equal(obs[:, 0], mc.mountaincar_cont_reset_state(2, np.arange(1), np.ones(1)))


def test_header_constants_equal_native():
    from openrl_amd import _native as n
    from openrl_amd import ops

    text = open(os.path.join(ROOT, "include", "orl_hip.h")).read()
    m = re.search(r"#define ORL_ENV_MOUNTAINCAR_CONT (\d+)", text)
    assert m and int(m.group(1)) == n.ORL_ENV_MOUNTAINCAR_CONT == ops.ENV_MOUNTAINCAR_CONT == 8
    assert n.ORL_VERSION == 306
    env_h = open(os.path.join(ROOT, "openrl_amd", "csrc", "orl_env.h")).read()
    assert re.search(r"MOUNTAINCAR_CONT_STATE_W = %d;" % mc.MOUNTAINCAR_CONT_STATE_W, env_h)
    assert "0x%Xu" % mc.MOUNTAINCAR_CONT_KEY in env_h and "0x3C4A0000u" in env_h


def test_state_width_and_fused_rollout_argument_checks():
    """The fused rollout takes a Gaussian head with one output and 2-d observations, on the chain kernel only: every
    other request returns ORL_E_INVALID with a message before anything is launched."""
    from openrl_amd import _native as n

    lib = n.load()
    kind = n.ORL_ENV_MOUNTAINCAR_CONT
    assert lib.orl_env_state_width(kind) == 4
    fake = 4096  # non-null placeholders: validation fails before any pointer is used
    buf = n.BufferPtrs()
    for f in ("policy_obs", "critic_obs", "rewards", "masks", "bad_masks", "active_masks"):
        setattr(buf, f, fake)
    buf.T, buf.N, buf.A, buf.Dp, buf.Dc = 8, 16, 1, 2, 2
    args = n.RolloutArgs(buf, fake, fake, fake, fake, fake, kind, 999, 1, 2, 0)
    cri = n.NetDesc(2, 64, 1, n.ORL_HEAD_VALUE)
    for pol in (n.NetDesc(2, 64, 3, n.ORL_HEAD_CATEGORICAL), n.NetDesc(2, 64, 2, n.ORL_HEAD_GAUSSIAN)):
        rc = lib.orl_rollout_fused(C.byref(pol), C.c_void_p(fake), C.byref(cri), C.c_void_p(fake), C.byref(args), None, None)
        assert rc == -1 and b"MountainCarContinuous" in lib.orl_last_error_string()
    buf.Dp = buf.Dc = 3
    args = n.RolloutArgs(buf, fake, fake, fake, fake, fake, kind, 999, 1, 2, 0)
    pol, cri3 = n.NetDesc(3, 64, 1, n.ORL_HEAD_GAUSSIAN), n.NetDesc(3, 64, 1, n.ORL_HEAD_VALUE)
    rc = lib.orl_rollout_fused(C.byref(pol), C.c_void_p(fake), C.byref(cri3), C.c_void_p(fake), C.byref(args), None, None)
    assert rc == -1 and b"MountainCarContinuous" in lib.orl_last_error_string()
    buf.Dp = buf.Dc = 2
    args = n.RolloutArgs(buf, fake, fake, fake, fake, fake, kind, 999, 1, 2, 0)
    args.opp_reserved = 1
    pol = n.NetDesc(2, 64, 1, n.ORL_HEAD_GAUSSIAN)
    rc = lib.orl_rollout_fused(C.byref(pol), C.c_void_p(fake), C.byref(cri), C.c_void_p(fake), C.byref(args), None, None)
    assert rc == -1 and b"lockstep" in lib.orl_last_error_string()
    # the stand-alone kernels check their widths before launching
    assert lib.orl_env_reset(kind, C.c_void_p(fake), None, C.c_void_p(fake), 4, 3, 0, 999, None) == -1
    assert b"MountainCarContinuous" in lib.orl_last_error_string()


def test_make_needs_a_gpu():
    from openrl_amd import _native as nat
    from openrl_amd.envs.common import make

    with pytest.raises(nat.NativeError):
        make("MountainCarContinuous-v0", env_num=2, seed=0)


def test_cpu_port_iteration_on_the_oracle_env():
    from tests.pendulum_oracle import GaussianCPUTrainer

    N, T = 8, 16
    tr = GaussianCPUTrainer(N, T, mc.MountainCarContinuousEnvOracle(N, 0), obs_dim=2, n_actions=1, seed=0, ppo_epoch=2,
                            threads=2)
    th0 = tr.ptheta.clone()
    tr.rollout()
    b = tr.buf
    assert b.policy_obs.shape == (T + 1, N, 1, 2) and b.actions.shape == (T, N, 1, 1)
    np.testing.assert_array_equal(b.rewards[:, :, 0, 0], -((b.actions[:, :, 0, 0] ** 2).astype(f32) * f32(0.1)))
    info = tr.update()
    assert np.isfinite(info["policy_loss"]) and not np.array_equal(th0.numpy(), tr.ptheta.numpy())
