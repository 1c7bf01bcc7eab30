"""Pendulum-v1 on a MI355X (ORL_ENV_PENDULUM): the stand-alone env kernels against the fp32 restatement
(tests/pendulum_oracle.py pendulum_step_f32), the chain rollout kernel (csrc/orl_rollout2.h) against the stepwise route and
per step against the oracle, the towers teacher-forced, the reference's Pendulum callback segment, learning next to the
CPU port, and the stepwise / hipGraph routes of general and recurrent towers."""
import numpy as np
import pytest
import torch

from oracle import philox as px
from oracle import ppo_oracle as po
from tests import pendulum_oracle as pend

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cfg(argv=()):
    from openrl_amd.configs.config import default_cfg

    return default_cfg(list(argv))


def _build(N, T, seed=3, argv=()):
    from openrl_amd.algorithms.ppo import PPOAlgorithm
    from openrl_amd.buffers import NormalReplayBuffer
    from openrl_amd.envs.common import make
    from openrl_amd.modules.common import PPONet

    cfg = _cfg(["--seed", str(seed), "--episode_length", str(T)] + list(argv))
    env = make("Pendulum-v1", env_num=N, device=DEV, seed=seed)
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


def test_env_kernels_teacher_forced_against_the_restatement():
    """512 envs, random actions in [-5, 5] (the torque clip), 450 steps = two auto-resets: every step's observation,
    reward and state from the device's own previous state; done exactly at steps 200 and 400; reset states keyed."""
    from openrl_amd.envs.common import make

    N, seed = 512, 11
    env = make("Pendulum-v1", env_num=N, seed=seed, device=DEV)
    obs, _ = env.reset(seed=seed)
    s0 = pend.pendulum_reset_state(seed, np.arange(N), np.zeros(N))
    np.testing.assert_array_equal(env.env_state[:, :2].cpu().numpy(), s0)
    np.testing.assert_allclose(obs[:, 0], pend.pendulum_obs_f32(s0), rtol=2e-5, atol=2e-6)
    assert env.observation_space.contains(obs[0, 0])
    rs = np.random.RandomState(0)
    for t in range(1, 451):
        state = env.env_state[:, :2].cpu().numpy().copy()
        a = rs.uniform(-5, 5, N).astype(np.float32)
        o, r, d, _ = env.step(a.reshape(N, 1, 1))
        nxt, oo, rr = pend.pendulum_step_f32(state, a)
        np.testing.assert_allclose(r[:, 0, 0], rr, rtol=2e-5, atol=2e-6)
        assert np.all(d[:, 0] == (t % 200 == 0)), t
        st = env.env_state.cpu().numpy()
        if t % 200 == 0:
            fresh = pend.pendulum_reset_state(seed, np.arange(N), np.full(N, t // 200))
            np.testing.assert_array_equal(st[:, :2], fresh)
            np.testing.assert_allclose(o[:, 0], pend.pendulum_obs_f32(fresh), rtol=2e-5, atol=2e-6)
            assert np.all(st[:, 2] == 0) and np.all(st[:, 3] == t // 200)
        else:
            np.testing.assert_allclose(st[:, :2], nxt, rtol=2e-5, atol=2e-6)
            np.testing.assert_allclose(o[:, 0], oo, rtol=2e-5, atol=2e-6)
            assert np.all(st[:, 2] == t % 200)
        assert np.all(np.abs(st[:, 0]) <= np.pi + 1e-6)


def _check_chain_steps_against_oracle(d, seed, ep0):
    """Per step of a chain rollout: (obs_t, action_t) -> obs_{t+1}, reward_t through pendulum_step_f32 from
    th = atan2(o1, o0), thdot = o2; an auto-reset step's next observation is the keyed reset state's."""
    obs = d["policy_obs"][:, :, 0]
    act, rew, masks = d["actions"][:, :, 0, 0], d["rewards"][:, :, 0, 0], d["masks"][:, :, 0, 0]
    T, N = act.shape
    ep = ep0.copy()
    for t in range(T):
        st = np.stack([np.arctan2(obs[t, :, 1], obs[t, :, 0]), obs[t, :, 2]], axis=-1).astype(np.float32)
        _, oo, rr = pend.pendulum_step_f32(st, act[t])
        np.testing.assert_allclose(rew[t], rr, rtol=2e-5, atol=5e-6, err_msg="reward t=%d" % t)
        live = masks[t + 1] != 0
        np.testing.assert_allclose(obs[t + 1][live], oo[live], rtol=2e-5, atol=5e-6, err_msg="obs t=%d" % t)
        if (~live).any():
            ep = ep + (~live)
            fresh = pend.pendulum_obs_f32(pend.pendulum_reset_state(seed, np.arange(N), ep))
            np.testing.assert_allclose(obs[t + 1][~live], fresh[~live], rtol=2e-5, atol=2e-6)
    return ep


@pytest.mark.parametrize("N,T", [(50, 23), (4096, 200), (17, 2)])
def test_chain_rollout_equals_stepwise_and_steps_like_the_oracle(N, T):
    """The chain kernel (fused) and the stepwise route on the same seeds, two consecutive rollouts (env_state / ep_stats
    carry over).  (17, 2): fewer envs than a tile, fewer steps than the rings are deep.

    The env arithmetic of the two routes is the same code (orl_env.h, explicit fmaf), but their towers round differently
    (head from LayerNorm-2 partials on the chain), and the closed loop policy -> torque -> state amplifies those ulps over a
    200-step episode.  Measured at 4096 x 200: the largest action difference of the first rollout was 9.5e-6 absolute (6
    of 819 200 actions outside rtol 1e-5 / atol 2e-6; the largest relative difference per 50 steps grew 2e-4 -> 8e-3).
    The values differ more (the chain's critic is the fp16 two-term split sweep, evaluated on the drifted observations):
    4.5e-5 at most in the first 50 steps, 1.3e-3 over the whole rollout.  So the first rollout's first 50 steps are
    compared at rtol 1e-5 (actions) / 1e-4 (values, observations, rewards); over both whole rollouts 99.99 % of the
    actions must agree to 1e-5 of the action scale (std ~ 1) and all to 2e-3 (the second rollout, measured: 13 of 819 200
    beyond 1e-5, the largest 2.6e-4), the log-probs to 1e-4.  The per-step check against the oracle below is exact per step and
    carries the correctness of the in-kernel env at full size; the values of the chain's own observations are pinned
    against the oracle towers by test_chain_rollout_teacher_forced_vs_oracle_towers."""
    seed = 3
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
        dev = np.abs(a["actions"] - b["actions"]) / (np.abs(b["actions"]) + 1e-6)
        print("rollout %d: max relative action difference per 50 steps %s" % (k, [float(dev[i:i + 50].max())
                                                                               for i in range(0, T, 50)]))
        h = 50 if k == 0 else 0  # (the second rollout starts from states the routes reached on their own)
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
    assert np.array_equal(sa[:, 2:], sb[:, 2:]) and np.array_equal(sa[:, 3], ep.astype(np.float32))
    assert np.array_equal(ea[:, 1::2], eb[:, 1::2])  # episode lengths and counts
    np.testing.assert_allclose(ea[:, 0::2], eb[:, 0::2], rtol=1e-3, atol=1e-2)  # returns


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
    pspec, cspec = po.TowerSpec(3, 1, po.HEAD_GAUSSIAN), po.TowerSpec(3, 1, po.HEAD_VALUE)
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


def test_reference_pendulum_callback_segment():
    """tests/test_callbacks/test_callbacks.py:112-128 of the reference, imports swapped: StopTrainingOnMaxEpisodes(1) on
    Pendulum-v1 with 2 envs stops after one 200-step episode per env."""
    from openrl_amd.configs.config import create_config_parser
    from openrl_amd.envs.common import make
    from openrl_amd.modules.common import PPONet as Net
    from openrl_amd.runners.common import PPOAgent as Agent
    from openrl_amd.utils.callbacks import CallbackList, StopTrainingOnMaxEpisodes

    config = create_config_parser().parse_args(["--seed", "0"])
    max_episodes = 1
    n_envs = 2
    max_episode_length = 200
    env = make("Pendulum-v1", env_num=n_envs)
    obs, _ = env.reset(seed=0)
    assert env.observation_space.contains(obs[0, 0]) and env.observation_space.contains(obs[1, 0])
    agent = Agent(Net(env, cfg=config))
    callback_max_episodes = StopTrainingOnMaxEpisodes(max_episodes=max_episodes, verbose=1)
    callback = CallbackList([callback_max_episodes])
    agent.train(1000, callback=callback)
    episodes_per_env = callback_max_episodes.n_episodes // n_envs
    assert episodes_per_env == max_episodes
    time_steps_per_env = agent.num_time_steps // n_envs
    assert time_steps_per_env == max_episode_length
    env.close()


LEARN_N, LEARN_T, LEARN_ITERS, LEARN_SEEDS = 64, 200, 60, (0, 1, 2)
LEARN_ARGV = ["--gamma", "0.9"]
LEARN_FLOOR = 700.0


def _gain(curve):
    return float(np.mean(curve[-3:]) - np.mean(curve[:3]))


def _learn_engine(seed):
    cfg, env, net, trainer, buf, agent = _build(LEARN_N, LEARN_T, seed=seed, argv=LEARN_ARGV + ["--log_interval", "1000000"])
    cfg.num_env_steps = LEARN_N * LEARN_T * LEARN_ITERS
    drv = _driver(cfg, env, trainer, buf, agent)
    assert drv.fused
    drv.reset_and_buffer_init()
    curve = []
    for i in range(LEARN_ITERS):
        drv.episode = i
        drv._inner_loop()
        curve.append(float(buf.data.rewards[:, :, 0, 0].sum(0).mean()))
    return curve


def _learn_port(seed):
    tr = pend.GaussianCPUTrainer(LEARN_N, LEARN_T, pend.PendulumEnvOracle(LEARN_N, seed), obs_dim=3, n_actions=1, seed=seed,
                                 ppo_epoch=10, num_mini_batch=1, gamma=0.9, threads=8)
    curve = []
    for _ in range(LEARN_ITERS):
        tr.iterate()
        curve.append(float(tr.buf.rewards.sum(0).mean()))
    return curve


def test_pendulum_learning_engine_vs_cpu_port():
    """Engine (fused chain rollout) and the CPU port of the reference's maths on the same restated env, 3 seeds, 64 envs x
    200 steps (one episode per env and iteration) x 60 iterations, --gamma 0.9 on both sides.  Score: the mean episode
    return of the last 3 iterations minus the first 3.  Engine median gain >= 0.85 x the port's, smallest engine gain >=
    LEARN_FLOOR.  A random policy scores about -1 200 per episode.

    Measured on a MI355X (mean episode return every 5th iteration, then the last):
        seed 0 engine -1306 -1067 -862 -411 -269 -183 -200 -204 -205 -197 -169 -208 -184
               port   -1314 -1054 -852 -492 -278 -198 -209 -208 -222 -219 -180 -207 -188
        seed 1 engine -1273 -1159 -888 -394 -277 -228 -185 -208 -176 -160 -181 -196 -173
               port   -1301 -1108 -888 -472 -366 -265 -204 -209 -189 -161 -196 -201 -180
        seed 2 engine -1195 -1066 -919 -502 -278 -245 -177 -213 -178 -183 -182 -209 -196
               port   -1213 -1062 -872 -510 -324 -278 -197 -213 -184 -192 -187 -214 -200
    gains: engine 1038.6 / 1046.4 / 1026.1, port 1021.9 / 1033.2 / 1008.6.  Both sides plateau near -190 after ~30
    iterations.  The default gamma 0.99 was not run on the GPU; gamma 0.9 is a common Pendulum setting (a 200-step
    horizon of dense costs).  The floor (700) leaves ~30 % margin under the smallest measured
    engine gain."""
    eng = [_learn_engine(s) for s in LEARN_SEEDS]
    port = [_learn_port(s) for s in LEARN_SEEDS]
    ge, gp = [_gain(c) for c in eng], [_gain(c) for c in port]
    for s, ce, cp in zip(LEARN_SEEDS, eng, port):
        print("seed %d engine %s" % (s, [round(x) for x in ce[::5]] + [round(ce[-1])]))
        print("seed %d port   %s" % (s, [round(x) for x in cp[::5]] + [round(cp[-1])]))
    print("gains: engine %s port %s" % ([round(g, 1) for g in ge], [round(g, 1) for g in gp]))
    assert np.median(ge) >= 0.85 * np.median(gp), (ge, gp)
    assert min(ge) >= LEARN_FLOOR, (ge, gp)


@pytest.mark.parametrize("argv", [["--hidden_size", "128"], ["--use_recurrent_policy", "true"]])
def test_general_and_recurrent_towers_train_stepwise_and_graph_replayed(argv):
    """Towers outside the fused instances roll out on Pendulum through the stepwise route: the first rollout eagerly, the
    second replayed from the captured hipGraph (the env step's counter has a device part); two iterations train."""
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
    assert np.all(st[:, 2] == (2 * T) % 200) and np.all(np.abs(st[:, 0]) <= np.pi + 1e-6)
    for k, m in net.module.models.items():
        if th0[k] is not None:
            assert not torch.equal(th0[k], m.theta.detach())


def test_lockstep_kernel_is_refused_with_a_message():
    from openrl_amd import _native as nat

    cfg, env, net, trainer, buf, agent = _build(32, 8)
    cfg.amd_rollout_kernel = "lockstep"
    drv = _driver(cfg, env, trainer, buf, agent)
    drv.reset_and_buffer_init()
    with pytest.raises(nat.NativeError, match="lockstep"):
        drv.actor_rollout()


def test_deterministic_act_returns_the_mean():
    from openrl_amd.envs.common import make
    from openrl_amd.modules.common import PPONet as Net
    from openrl_amd.runners.common import PPOAgent as Agent

    N = 6
    env = make("Pendulum-v1", env_num=N, device=DEV, seed=2)
    agent = Agent(Net(env, cfg=_cfg(["--seed", "2"])))
    obs, _ = env.reset(seed=2)
    action, _ = agent.act(obs, deterministic=True)
    assert action.shape == (N, 1, 1)
    mod = agent.net.module
    spec = po.TowerSpec(3, 1, po.HEAD_GAUSSIAN)
    mean = po.tower_forward(spec, mod.models["policy"].theta.detach().cpu(), torch.as_tensor(obs[:, 0])).numpy()
    np.testing.assert_allclose(action[:, 0], mean, rtol=1e-4, atol=1e-5)
