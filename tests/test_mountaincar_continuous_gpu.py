"""MountainCarContinuous-v0 on a MI355X (ORL_ENV_MOUNTAINCAR_CONT): the stand-alone env kernels against the fp32
restatement (tests/mountaincar_continuous_oracle.py) over terminations and truncations, the chain rollout kernel
(csrc/orl_rollout2.h: MountainCar's pre / post split under the Gaussian head, the reward on the raw sample) against the
stand-alone step kernel bit for bit, its towers teacher-forced against the oracle towers, the fused route next to the
stepwise one, a scripted policy through the fused rollout, the stepwise / hipGraph routes of general and recurrent towers,
the lock-step kernel's refusal, and learning next to the CPU port."""
import numpy as np
import pytest
import torch

from oracle import philox as px
from oracle import ppo_oracle as po
from tests import mountaincar_continuous_oracle as mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENV_ID = "MountainCarContinuous-v0"
f32 = np.float32


@pytest.fixture(autouse=True)
def _leave_the_global_rngs_as_found():
    """Tower initialisation and the CPU port draw from the process-wide generators (random, numpy, torch), and the CPU
    port sets torch's thread count; later tests in the same process draw their initial weights from them (orthogonal
    initialisation's QR rounds differently with other thread counts), so every test here leaves them as it found them."""
    import random

    threads = torch.get_num_threads()
    state = (random.getstate(), np.random.get_state(), torch.get_rng_state(),
             torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None)
    yield
    random.setstate(state[0]); np.random.set_state(state[1]); torch.set_rng_state(state[2])
    torch.set_num_threads(threads)
    if state[3] is not None:
        torch.cuda.set_rng_state_all(state[3])


def _cfg(argv=()):
    from openrl_amd.configs.config import default_cfg

    return default_cfg(list(argv))


def _build(N, T, seed=3, argv=(), **env_kw):
    from openrl_amd.algorithms.ppo import PPOAlgorithm
    from openrl_amd.buffers import NormalReplayBuffer
    from openrl_amd.envs.common import make
    from openrl_amd.modules.common import PPONet

    cfg = _cfg(["--seed", str(seed), "--episode_length", str(T)] + list(argv))
    env = make(ENV_ID, env_num=N, device=DEV, seed=seed, **env_kw)
    net = PPONet(env, cfg=cfg, device=DEV, n_rollout_threads=N)

    class _Agent:
        num_time_steps = 0

    cfg.num_env_steps = N * T
    trainer = PPOAlgorithm(cfg, net.module, agent_num=1, device=DEV)
    buf = NormalReplayBuffer(cfg, 1, env.observation_space, env.action_space, device=DEV)
    return cfg, env, net, trainer, buf, _Agent()


def _driver(cfg, env, trainer, buf, agent):
    from openrl_amd.drivers.onpolicy_driver import OnPolicyDriver

    return OnPolicyDriver({"cfg": cfg, "num_agents": 1, "run_dir": None, "envs": env, "device": DEV}, trainer, buf, agent)


def _set_start_states(env, buf, st2):
    """Overwrite the envs' (position, velocity) and the buffer's first observation (the observation is the state)."""
    st = env.env_state.cpu().numpy()
    st[:, :2] = st2
    env.env_state.copy_(torch.from_numpy(st))
    buf.data.policy_obs[0, :, 0].copy_(torch.from_numpy(st2.astype(f32)))
    if buf.data.critic_obs is not buf.data.policy_obs:
        buf.data.critic_obs[0, :, 0].copy_(torch.from_numpy(st2.astype(f32)))


def _near_goal_and_wall(N, rs):
    """A third a step or two from the goal, a third at the left wall moving left, the rest from the usual start range."""
    k = N // 3
    st = np.stack([rs.uniform(-0.6, -0.4, N), np.zeros(N)], axis=-1)
    st[:k] = np.stack([rs.uniform(0.42, 0.449, k), rs.uniform(0.02, 0.05, k)], axis=-1)
    st[k:2 * k] = np.stack([rs.uniform(-1.2, -1.17, k), rs.uniform(-0.07, -0.01, k)], axis=-1)
    st[k] = (-1.2, -0.02)
    return st.astype(f32)


def test_make_spaces_and_random_action():
    from openrl_amd.envs.common import make

    env = make(ENV_ID, env_num=4, seed=0, device=DEV)
    assert env.kind == "mountaincar_continuous" and env.episode_limit == 999
    assert env.action_space.shape == (1,)
    np.testing.assert_array_equal(env.action_space.low, [-1.0])
    np.testing.assert_array_equal(env.action_space.high, [1.0])
    np.testing.assert_array_equal(env.observation_space.low, np.array([-1.2, -0.07], f32))
    np.testing.assert_array_equal(env.observation_space.high, np.array([0.6, 0.07], f32))
    obs, _ = env.reset(seed=1)
    assert all(env.observation_space.contains(o) for o in obs[:, 0])
    np.testing.assert_array_equal(obs[:, 0], mc.mountaincar_cont_reset_state(1, np.arange(4), np.zeros(4)))
    ra = env.random_action()
    assert ra.shape == (4, 1, 1) and np.all(np.abs(ra) <= 1.0)
    assert make(ENV_ID, env_num=2, seed=0, device=DEV, episode_limit=60).episode_limit == 60


def test_env_kernels_teacher_forced_against_the_restatement():
    """512 envs with episode_limit 60 for 150 steps: a third start a step or two from the goal and terminate at once, a
    third at the left wall, and every env is truncated at least twice.  Actions U(-2.5, 2.5) (the force clip; the reward
    takes the raw value).  Every step's next state, observation and reward from the device's own previous state through
    the fp32 restatement (tolerance 2e-5 relative / 2e-6 absolute on the state: the device's cos against numpy's), the
    terminal flag exact (the reward shows it: > 50 only with the bonus) except within 1e-6 of the goal, done exact, and
    every reset state exactly the keyed one."""
    from openrl_amd.envs.common import make

    N, seed, limit, steps = 512, 11, 60, 150
    env = make(ENV_ID, env_num=N, seed=seed, device=DEV, episode_limit=limit)
    obs, _ = env.reset(seed=seed)
    np.testing.assert_array_equal(env.env_state[:, :2].cpu().numpy(),
                                  mc.mountaincar_cont_reset_state(seed, np.arange(N), np.zeros(N)))
    rs = np.random.RandomState(0)
    st = env.env_state.cpu().numpy()
    st[:, :2] = _near_goal_and_wall(N, rs)
    env.env_state.copy_(torch.from_numpy(st))
    episode = np.zeros(N, np.int64)
    steps_in = np.zeros(N, np.int64)
    n_term = n_trunc = 0
    for t in range(1, steps + 1):
        state = env.env_state[:, :2].cpu().numpy().copy()
        a = rs.uniform(-2.5, 2.5, N).astype(f32)
        o, r, d, _ = env.step(a.reshape(N, 1, 1))
        stn = env.env_state.cpu().numpy()
        nxt, term, rr = mc.mountaincar_cont_step_f32(state, a)
        dev_term = r[:, 0, 0] > 50.0
        sure = ~((np.abs(nxt[:, 0] - mc.GOAL) < 1e-6) | (np.abs(nxt[:, 1]) < 1e-9))
        assert np.array_equal(dev_term[sure], term[sure]), t
        np.testing.assert_allclose(r[:, 0, 0], mc.mountaincar_cont_reward_f32(dev_term, a), rtol=0, atol=0)
        np.testing.assert_allclose(r[sure, 0, 0], rr[sure], rtol=1e-6, atol=1e-7)
        steps_in = steps_in + 1
        done = dev_term | (steps_in >= limit)
        assert np.array_equal(d[:, 0], done), t
        n_term += int(dev_term.sum())
        n_trunc += int((done & ~dev_term).sum())
        live = ~done
        np.testing.assert_allclose(stn[live, :2], nxt[live], rtol=2e-5, atol=2e-6, err_msg="state t=%d" % t)
        np.testing.assert_array_equal(o[live, 0], stn[live, :2])
        if done.any():
            episode = episode + done
            fresh = mc.mountaincar_cont_reset_state(seed, np.arange(N), episode)
            np.testing.assert_array_equal(stn[done, :2], fresh[done])
            np.testing.assert_array_equal(o[done, 0], fresh[done])
        steps_in = np.where(done, 0, steps_in)
        np.testing.assert_array_equal(stn[:, 2], steps_in.astype(f32))
        np.testing.assert_array_equal(stn[:, 3], episode.astype(f32))
    print("MountainCarContinuous: %d terminations, %d truncations in %d x %d random steps" % (n_term, n_trunc, N, steps))
    assert n_term >= N // 3 and episode.min() >= 2


def _replay_on_the_step_kernel(env, st0, ep0, d, D=2):
    """Replay the rollout's recorded actions through orl_env_step from the copied state: the observations, rewards and
    dones the stand-alone kernel produces, and its final state / statistics."""
    from openrl_amd import ops

    N = env.parallel_env_num
    st, ep = st0.clone(), ep0.clone()
    obs = torch.zeros(N, D, dtype=torch.float32, device=DEV)
    rew = torch.zeros(N, dtype=torch.float32, device=DEV)
    done = torch.zeros(N, dtype=torch.uint8, device=DEV)
    T = d.actions.shape[0]
    o_all, r_all, d_all = [], [], []
    for t in range(T):
        a = d.actions[t, :, 0].contiguous()
        ops.env_step(env.env_kind, st, ep, a, obs, rew, done, N, D, env.seed, env.episode_limit, t)
        o_all.append(obs.cpu().numpy().copy())
        r_all.append(rew.cpu().numpy().copy())
        d_all.append(done.cpu().numpy().copy())
    return np.stack(o_all), np.stack(r_all), np.stack(d_all), st.cpu().numpy(), ep.cpu().numpy()


def _assert_same_as_step_kernel(env, buf, st0, ep0, tag):
    d = buf.data
    o, r, dn, st, ep = _replay_on_the_step_kernel(env, st0, ep0, d)
    assert np.array_equal(d.policy_obs[1:, :, 0].cpu().numpy(), o), tag
    assert np.array_equal(d.rewards[:, :, 0, 0].cpu().numpy(), r), tag
    assert np.array_equal(d.masks[1:, :, 0, 0].cpu().numpy(), (dn == 0).astype(f32)), tag
    assert np.array_equal(env.env_state.cpu().numpy(), st), tag
    assert np.array_equal(env.ep_stats.cpu().numpy(), ep), tag
    return int(dn.sum()), int((r > 50).sum())


@pytest.mark.parametrize("N,T,near", [(50, 37, False), (4096, 200, False), (17, 2, False), (70, 64, True),
                                      (4096, 64, True)])
def test_chain_rollout_equals_the_step_kernel_bit_for_bit(N, T, near):
    """Two consecutive fused rollouts on the chain kernel; before each, env_state / ep_stats are copied, and the rollout's
    recorded actions (the raw Gaussian samples) are replayed through the stand-alone step kernel from the copy.
    Observations, rewards, masks and the final env_state / ep_stats must be IDENTICAL: this pins the pre / post split
    (the gravity term and the reset state on the env service wave, the force clip, the terminal test and the reward on
    wave 0), independently of how the towers round.  (17, 2): fewer envs than a tile, fewer steps than the rings are deep.
    ``near``: a third of the envs start a step or two from the goal and a third at the left wall moving left, so the
    terminal step, its +100 and the auto-reset are compared as well."""
    cfg, env, net, trainer, buf, agent = _build(N, T, seed=4)
    drv = _driver(cfg, env, trainer, buf, agent)
    assert drv.fused
    drv.reset_and_buffer_init()
    if near:
        _set_start_states(env, buf, _near_goal_and_wall(N, np.random.RandomState(1)))
    dones = terms = 0
    for k in range(2):
        st0, ep0 = env.env_state.clone(), env.ep_stats.clone()
        drv.actor_rollout()
        dn, tm = _assert_same_as_step_kernel(env, buf, st0, ep0, k)
        dones += dn
        terms += tm
        drv.compute_returns()
        buf.data.after_update()
    print("%d x %d (near %s): %d dones, %d terminations over two rollouts" % (N, T, near, dones, terms))
    if near:
        assert terms >= N // 3


def test_chain_rollout_teacher_forced_vs_oracle_towers():
    """4096 x 200 on the chain kernel, every 8th step: values and log-probs against po.get_actions with the Gaussian head
    and the same Philox normals (wave 5's: box_muller(x, y) of philox(act_seed, n, 0, step, 0)); actions = mean + std eps."""
    N, T = 4096, 200
    cfg, env, net, trainer, buf, agent = _build(N, T, seed=5)
    drv = _driver(cfg, env, trainer, buf, agent)
    assert drv.fused
    mod = net.module
    step0 = int(mod.rng_step)
    drv.reset_and_buffer_init()
    drv.actor_rollout()
    d = buf.data
    pspec, cspec = po.TowerSpec(2, 1, po.HEAD_GAUSSIAN), po.TowerSpec(2, 1, po.HEAD_VALUE)
    tp, tc = mod.models["policy"].theta.cpu(), mod.models["critic"].theta.cpu()
    obs = d.policy_obs.cpu().numpy()
    n = np.arange(N, dtype=np.uint32)
    for t in range(0, T, 8):
        x, y, _, _ = px.philox4x32_10(mod.act_seed, n, 0, step0 + t, 0)
        eps, _ = px.box_muller(x, y)
        v, a, lp = po.get_actions(pspec, tp, cspec, tc, obs[t, :, 0], obs[t, :, 0], None, False, eps.reshape(N, 1))
        np.testing.assert_allclose(d.value_preds[t, :, 0].cpu().numpy(), v, rtol=1e-4, atol=1e-5, err_msg="t=%d" % t)
        np.testing.assert_allclose(d.actions[t, :, 0].cpu().numpy(), a, rtol=1e-5, atol=2e-6, err_msg="t=%d" % t)
        np.testing.assert_allclose(d.action_log_probs[t, :, 0].cpu().numpy(), lp, rtol=1e-4, atol=1e-5, err_msg="t=%d" % t)


def _check_chain_steps_against_oracle(d, seed, ep0):
    """Per step of a rollout: (obs_t, action_t) -> obs_{t+1}, reward_t through the fp32 restatement; an auto-reset step's
    next observation is the keyed reset state's."""
    obs = d["policy_obs"][:, :, 0]
    act, rew, masks = d["actions"][:, :, 0, 0], d["rewards"][:, :, 0, 0], d["masks"][:, :, 0, 0]
    T, N = act.shape
    ep = ep0.copy()
    for t in range(T):
        nxt, term, rr = mc.mountaincar_cont_step_f32(obs[t], act[t])
        np.testing.assert_allclose(rew[t], rr, rtol=1e-6, atol=1e-7, err_msg="reward t=%d" % t)
        live = masks[t + 1] != 0
        np.testing.assert_allclose(obs[t + 1][live], nxt[live], rtol=2e-5, atol=2e-6, err_msg="obs t=%d" % t)
        if (~live).any():
            ep = ep + (~live)
            fresh = mc.mountaincar_cont_reset_state(seed, np.arange(N), ep)
            np.testing.assert_array_equal(obs[t + 1][~live], fresh[~live])
    return ep


def test_fused_against_stepwise_route():
    """The chain kernel (fused) and the stepwise route on the same seeds, 512 x 200, two consecutive rollouts (env_state /
    ep_stats carry over: the 999-step episodes span rollouts).  The env arithmetic of the two routes is one code (the
    bit-exact test above); the towers round differently (the chain's head from LayerNorm-2 partials, its critic an fp16
    two-term split), and the closed loop policy -> force -> state carries those ulps along.  The first rollout's first 50
    steps are compared at rtol 1e-5 (actions) / 1e-4 (values, observations, rewards); over both rollouts 99.99 % of the
    actions must agree to 1e-5 and all to 2e-3, the log-probs to 1e-4, the masks exactly.  Every step of the fused
    rollouts is also checked against the fp32 restatement.  Measured on a MI355X: the largest action difference was
    2.4e-7 in the first rollout and 5.4e-7 in the second, the largest value difference 9.5e-7 and 3.5e-5 (no episode
    ended: the policy is the untrained one)."""
    N, T, seed = 512, 200, 3
    bufs, finals = {}, {}
    for mode in ("fused", "stepwise"):
        cfg, env, net, trainer, buf, agent = _build(N, T, seed=seed)
        cfg.amd_rollout_mode = mode
        cfg.amd_use_graph = False
        drv = _driver(cfg, env, trainer, buf, agent)
        assert drv.fused == (mode == "fused")
        drv.reset_and_buffer_init()
        out = []
        for _ in range(2):
            drv.actor_rollout()
            drv.compute_returns()
            out.append({f: getattr(buf.data, f).cpu().numpy().copy() for f in
                        ("actions", "policy_obs", "rewards", "masks", "value_preds", "action_log_probs")})
            buf.data.after_update()
        bufs[mode] = out
        finals[mode] = (env.env_state.cpu().numpy().copy(), env.ep_stats.cpu().numpy().copy())
    ep = np.zeros(N, np.int64)
    for k in range(2):
        a, b = bufs["fused"][k], bufs["stepwise"][k]
        dev = np.abs(a["actions"] - b["actions"])
        print("rollout %d: max action difference per 50 steps %s, values %s" % (
            k, [float(dev[i:i + 50].max()) for i in range(0, T, 50)],
            [float(np.abs(a["value_preds"] - b["value_preds"])[i:i + 50].max()) for i in range(0, T, 50)]))
        h = 50 if k == 0 else 0
        np.testing.assert_allclose(a["actions"][:h], b["actions"][:h], rtol=1e-5, atol=2e-6)
        for f in ("value_preds", "policy_obs", "rewards"):
            np.testing.assert_allclose(a[f][:h], b[f][:h], rtol=1e-4, atol=1e-4, err_msg=f)
        close = np.isclose(a["actions"], b["actions"], rtol=1e-5, atol=1e-5)
        assert close.mean() >= 0.9999, close.mean()
        np.testing.assert_allclose(a["actions"], b["actions"], rtol=0, atol=2e-3)
        np.testing.assert_allclose(a["action_log_probs"], b["action_log_probs"], rtol=1e-4, atol=1e-4)
        assert np.array_equal(a["masks"], b["masks"])
        ep = _check_chain_steps_against_oracle(a, seed, ep)
    (sa, ea), (sb, eb) = finals["fused"], finals["stepwise"]
    assert np.array_equal(sa[:, 2:], sb[:, 2:]) and np.array_equal(sa[:, 3], ep.astype(f32))
    print("episodes ended over both rollouts: %d (the rest carry into the next rollout)" % int(sa[:, 3].sum()))
    assert np.array_equal(ea[:, 1::2], eb[:, 1::2])  # episode lengths and counts
    np.testing.assert_allclose(ea[:, 0::2], eb[:, 0::2], rtol=1e-3, atol=1e-2)  # returns


def _scripted_policy(theta, spec):
    """Default-tower parameters whose Gaussian head is ~+1 for v >= 0 and ~-1 for v < 0, with std exp(-30): fc1 feeds
    relu(+-1e8 v) into two features, LayerNorm 1 turns either into the same +-sqrt(63)-pattern whatever |v|, fc2's first
    feature is their difference plus 4 (so v = 0 counts as positive), LayerNorm 2 maps its sign to +-sqrt(63), and the
    head scales that by 1 / sqrt(63)."""
    th = torch.zeros_like(theta)
    p = spec.split(th)
    p["W1"][0, 1], p["W1"][1, 1] = 1e8, -1e8
    p["g1"].fill_(1.0); p["g2"].fill_(1.0)
    p["W2"][0, 0], p["W2"][0, 1] = 1.0, -1.0
    p["b2"][0] = 4.0
    p["W3"][0, 0] = 1.0 / np.sqrt(63.0)
    p["logstd"].fill_(-30.0)
    return th


def test_scripted_policy_through_the_fused_rollout_reaches_the_goal():
    """a = +1 if v >= 0 else -1 (to ~1e-4: a tower built for it, std exp(-30)) through orl_rollout_fused, 512 envs x 300
    steps from the usual start states: every env reaches the goal well within the 999-step limit, the terminal step pays
    100 - 0.1 a^2 (~99.9), the next observation is the oracle's start state of episode 1, and the oracle env driven with
    the recorded actions ends the same episodes on the same steps."""
    N, T, seed = 512, 300, 9
    cfg, env, net, trainer, buf, agent = _build(N, T, seed=seed)
    drv = _driver(cfg, env, trainer, buf, agent)
    assert drv.fused
    pol = net.module.models["policy"]
    with torch.no_grad():
        pol.theta.copy_(_scripted_policy(pol.theta.detach().cpu(), po.TowerSpec(2, 1, po.HEAD_GAUSSIAN)).to(DEV))
    drv.reset_and_buffer_init()
    drv.actor_rollout()
    d = buf.data
    obs, act = d.policy_obs[:, :, 0].cpu().numpy(), d.actions[:, :, 0, 0].cpu().numpy()
    rew, done = d.rewards[:, :, 0, 0].cpu().numpy(), d.masks[1:, :, 0, 0].cpu().numpy() == 0
    want = np.where(obs[:-1, :, 1] >= 0, 1.0, -1.0)
    np.testing.assert_allclose(act, want, rtol=0, atol=2e-4)
    assert done.any(axis=0).all(), np.flatnonzero(~done.any(axis=0))
    first = done.argmax(axis=0)
    n = np.arange(N)
    np.testing.assert_allclose(rew[first, n], 99.9, rtol=0, atol=1e-4)
    np.testing.assert_array_equal(rew[first, n], mc.mountaincar_cont_reward_f32(np.ones(N, bool), act[first, n]))
    np.testing.assert_array_equal(obs[first + 1, n], mc.mountaincar_cont_reset_state(seed, n, np.ones(N)))
    orc = mc.MountainCarContinuousEnvOracle(N, seed)
    np.testing.assert_array_equal(obs[0], orc.state)
    for t in range(T):
        o, r, od, _ = orc.step(act[t].reshape(N, 1, 1))
        assert np.array_equal(od[:, 0], done[t]), t
        np.testing.assert_allclose(obs[t + 1], o[:, 0], rtol=2e-5, atol=2e-6, err_msg="t=%d" % t)
    print("scripted MountainCarContinuous: first episode lengths min %d, mean %.1f, max %d" % (
        first.min() + 1, first.mean() + 1, first.max() + 1))
    assert first.max() + 1 < 300


@pytest.mark.parametrize("argv", [["--hidden_size", "128"], ["--use_recurrent_policy", "true"]])
def test_general_and_recurrent_towers_train_stepwise_and_graph_replayed(argv):
    """Towers outside the fused instances roll out through the stepwise route: the first rollout eagerly, the second
    replayed from the captured hipGraph (the env step's counter has a device part); two iterations train."""
    N, T = 32, 16
    cfg, env, net, trainer, buf, agent = _build(N, T, seed=1, argv=argv + ["--log_interval", "1000000"])
    drv = _driver(cfg, env, trainer, buf, agent)
    assert not drv.fused and drv._graph_ok
    drv.reset_and_buffer_init()
    th0 = {k: m.theta.detach().clone() if hasattr(m, "theta") else None for k, m in net.module.models.items()}
    for i in range(2):
        drv.episode = i
        assert drv._inner_loop()
    assert drv._graph is not None
    d = buf.data
    assert torch.isfinite(d.actions).all() and torch.isfinite(d.value_preds).all()
    assert (d.rewards <= 0).all()
    st = env.env_state.cpu().numpy()
    assert np.all(st[:, 2] == 2 * T) and np.all(st[:, 0] >= -1.2) and np.all(st[:, 0] <= 0.6)
    for k, m in net.module.models.items():
        if th0[k] is not None:
            assert not torch.equal(th0[k], m.theta.detach())


def test_lockstep_kernel_is_refused_with_a_message():
    from openrl_amd import _native as nat

    cfg, env, net, trainer, buf, agent = _build(32, 8)
    cfg.amd_rollout_kernel = "lockstep"
    drv = _driver(cfg, env, trainer, buf, agent)
    drv.reset_and_buffer_init()
    with pytest.raises(nat.NativeError, match="MountainCarContinuous.*lockstep"):
        drv.actor_rollout()
    # the next call (the chain kernel) still works
    cfg.amd_rollout_kernel = "chain"
    drv2 = _driver(cfg, env, trainer, buf, agent)
    drv2.reset_and_buffer_init()
    drv2.actor_rollout()
    assert torch.isfinite(buf.data.value_preds).all() and torch.isfinite(buf.data.rewards).all()


LEARN_N, LEARN_T, LEARN_ITERS, LEARN_SEEDS = 64, 200, 50, (0, 1, 2)
LEARN_RATIO, LEARN_FLOOR = 0.4, 0.25


def _gain(curve):
    return float(np.mean(curve[-3:]) - np.mean(curve[:3]))


def _learn_engine(seed):
    cfg, env, net, trainer, buf, agent = _build(LEARN_N, LEARN_T, seed=seed, argv=["--log_interval", "1000000"])
    cfg.num_env_steps = LEARN_N * LEARN_T * LEARN_ITERS
    drv = _driver(cfg, env, trainer, buf, agent)
    assert drv.fused
    drv.reset_and_buffer_init()
    curve = []
    for i in range(LEARN_ITERS):
        drv.episode = i
        drv._inner_loop()
        curve.append(float(buf.data.rewards[:, :, 0, 0].mean()))
    return curve


def _learn_port(seed):
    from tests.pendulum_oracle import GaussianCPUTrainer

    tr = GaussianCPUTrainer(LEARN_N, LEARN_T, mc.MountainCarContinuousEnvOracle(LEARN_N, seed), obs_dim=2, n_actions=1,
                            seed=seed, ppo_epoch=10, num_mini_batch=1, threads=8)
    curve = []
    for _ in range(LEARN_ITERS):
        tr.iterate()
        curve.append(float(tr.buf.rewards.mean()))
    return curve


def test_learning_engine_vs_cpu_port():
    """Engine (fused chain rollout, default recipe) and the CPU port of the reference's maths on the same restated env,
    3 seeds, 64 envs x 200 steps x 50 iterations (the 999-step episodes span rollouts).  Score: the mean per-step reward
    of the last 3 iterations minus the first 3.  A random N(0, 1) policy pays ~0.1 per step in action cost; PPO first
    shrinks that cost and then, at this budget, finds the goal (+100) on most seeds - but when is a matter of luck in
    the random streams, which the two sides do not share.  So the bar compares the gains, not the 90-point threshold:
    the engine's median gain >= LEARN_RATIO x the port's, and its smallest gain >= LEARN_FLOOR.

    Measured on a MI355X over seeds 0-7 at these settings (gains, engine / port):
        0.471 / 0.854, 0.719 / 0.704, 0.374 / 0.924, 0.678 / 0.685, 0.510 / 0.068, 0.574 / 0.387, 0.516 / 0.459,
        0.502 / 0.819
    engine median 0.51 (0.37 - 0.72), port median 0.70 (0.07 - 0.92): the same spread, one side ahead on some seeds and
    behind on others.  Seeds 0-2 (this test) give an engine median of 0.55 x the port's; the ratio 0.4 and the floor 0.25
    leave ~30 % margin under the measured values.  Mean per-step reward every 10th iteration, then the last:
        seed 0 engine -0.099 -0.092 -0.081 -0.064  0.147  0.386    port -0.100 -0.092  0.131  0.368  0.540  0.757
        seed 1 engine -0.099 -0.091 -0.010  0.227  0.387  0.667    port -0.099 -0.096  0.040  0.239  0.407  0.636
        seed 2 engine -0.101 -0.092 -0.086 -0.072  0.072  0.279    port -0.098 -0.078  0.096  0.330  0.544  0.825
    (37 s on the GPU, engine and CPU port together)."""
    eng = [_learn_engine(s) for s in LEARN_SEEDS]
    port = [_learn_port(s) for s in LEARN_SEEDS]
    ge, gp = [_gain(c) for c in eng], [_gain(c) for c in port]
    for s, ce, cp in zip(LEARN_SEEDS, eng, port):
        print("seed %d engine %s" % (s, [round(x, 4) for x in ce[::10]] + [round(ce[-1], 4)]))
        print("seed %d port   %s" % (s, [round(x, 4) for x in cp[::10]] + [round(cp[-1], 4)]))
    print("gains: engine %s port %s" % ([round(g, 4) for g in ge], [round(g, 4) for g in gp]))
    assert min(ge) >= LEARN_FLOOR, (ge, gp)
    assert np.median(ge) >= LEARN_RATIO * np.median(gp), (ge, gp)
