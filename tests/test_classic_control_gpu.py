"""Acrobot-v1 and MountainCar-v0 on a MI355X (ORL_ENV_ACROBOT / ORL_ENV_MOUNTAINCAR): the stand-alone env kernels
against the fp32 restatements (tests/classic_control_oracle.py), the chain rollout kernel (csrc/orl_rollout2.h: Acrobot's
speculative step, MountainCar's pre / post split) against the stand-alone step kernel bit for bit, its towers
teacher-forced against the oracle towers, the fused route next to the stepwise one, a scripted MountainCar policy, the
stepwise / hipGraph routes of general and recurrent towers, the lock-step kernel's refusal, and Acrobot learning next to
the CPU port."""
import numpy as np
import pytest
import torch

from oracle import philox as px
from oracle import ppo_oracle as po
from tests import classic_control_oracle as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENVS = {"acrobot": ("Acrobot-v1", 6, 500), "mountaincar": ("MountainCar-v0", 2, 200)}


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


def _build(which, N, T, seed=3, argv=()):
    from openrl_amd.algorithms.ppo import PPOAlgorithm
    from openrl_amd.buffers import NormalReplayBuffer
    from openrl_amd.envs.common import make
    from openrl_amd.modules.common import PPONet

    cfg = _cfg(["--seed", str(seed), "--episode_length", str(T)] + list(argv))
    env = make(ENVS[which][0], env_num=N, device=DEV, seed=seed)
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


def test_make_spaces_and_random_action():
    from openrl_amd.envs.common import make

    a = make("Acrobot-v1", env_num=4, seed=0, device=DEV)
    assert a.kind == "acrobot" and a.episode_limit == 500 and a.action_space.n == 3
    hi = np.array([1, 1, 1, 1, 4 * np.pi, 9 * np.pi], np.float32)
    np.testing.assert_array_equal(a.observation_space.high, hi)
    np.testing.assert_array_equal(a.observation_space.low, -hi)
    m = make("MountainCar-v0", env_num=4, seed=0, device=DEV)
    assert m.kind == "mountaincar" and m.episode_limit == 200 and m.action_space.n == 3
    np.testing.assert_array_equal(m.observation_space.low, np.array([-1.2, -0.07], np.float32))
    np.testing.assert_array_equal(m.observation_space.high, np.array([0.6, 0.07], np.float32))
    for env in (a, m):
        obs, _ = env.reset(seed=1)
        assert all(env.observation_space.contains(o) for o in obs[:, 0])
        ra = env.random_action()
        assert ra.shape == (4, 1, 1) and set(np.unique(ra).tolist()) <= {0, 1, 2}


@pytest.mark.parametrize("which,steps", [("acrobot", 1100), ("mountaincar", 450)])
def test_env_kernels_teacher_forced_against_the_restatement(which, steps):
    """512 envs, uniform random actions, past two truncations: every step's next state, observation and reward from the
    device's own previous state through the fp32 restatement (tolerance 2e-5 relative / 2e-6 absolute: the device's
    sin / cos / division against numpy's; the terminal test is compared exactly except within 1e-5 of its boundary),
    done exact, and every reset state exactly the keyed one."""
    from openrl_amd.envs.common import make

    N, seed = 512, 11
    name, D, limit = ENVS[which]
    env = make(name, env_num=N, seed=seed, device=DEV)
    obs, _ = env.reset(seed=seed)
    reset = cc.acrobot_reset_state if which == "acrobot" else cc.mountaincar_reset_state
    sw = 4 if which == "acrobot" else 2
    np.testing.assert_array_equal(env.env_state[:, :sw].cpu().numpy(), reset(seed, np.arange(N), np.zeros(N)))
    rs = np.random.RandomState(0)
    episode = np.zeros(N, np.int64)
    steps_in = np.zeros(N, np.int64)
    n_term = 0
    for t in range(1, steps + 1):
        state = env.env_state[:, :sw].cpu().numpy().copy()
        a = rs.randint(0, 3, N)
        o, r, d, _ = env.step(a.reshape(N, 1, 1))
        st = env.env_state.cpu().numpy()
        if which == "acrobot":
            nxt, oo, term, rr = cc.acrobot_step_f32(state, a)
            m = -np.cos(nxt[:, 0].astype(np.float64)) - np.cos(nxt[:, 0].astype(np.float64) + nxt[:, 1]) - 1.0
            sure = np.abs(m) > 1e-5
        else:
            nxt, term, rr = cc.mountaincar_step_f32(state, a)
            oo, sure = nxt, np.ones(N, bool)
        if which == "acrobot":
            dev_term = r[:, 0, 0] == 0.0
        else:  # (a termination on the truncating step itself is not visible apart from the truncation)
            sure = steps_in + 1 < limit
            dev_term = d[:, 0] & sure
        assert np.array_equal(dev_term[sure], term[sure]), t
        n_term += int(dev_term.sum())
        steps_in = steps_in + 1
        done = dev_term | (steps_in >= limit)
        assert np.array_equal(d[:, 0], done), t
        np.testing.assert_allclose(r[:, 0, 0], np.where(dev_term, 0.0, -1.0) if which == "acrobot" else -1.0)
        live = ~done
        np.testing.assert_allclose(st[live, :sw], nxt[live], rtol=2e-5, atol=2e-6, err_msg="state t=%d" % t)
        np.testing.assert_allclose(o[live, 0], oo[live], rtol=2e-5, atol=2e-6, err_msg="obs t=%d" % t)
        if done.any():
            episode = episode + done
            fresh = reset(seed, np.arange(N), episode)
            np.testing.assert_array_equal(st[done, :sw], fresh[done])
            fo = cc.acrobot_obs_f32(fresh) if which == "acrobot" else fresh
            np.testing.assert_allclose(o[done, 0], fo[done], rtol=2e-5, atol=2e-6)
        steps_in = np.where(done, 0, steps_in)
        np.testing.assert_array_equal(st[:, sw], steps_in.astype(np.float32))
        np.testing.assert_array_equal(st[:, sw + 1], episode.astype(np.float32))
    assert episode.min() >= 2
    print("%s: %d terminations in %d x %d random steps" % (which, n_term, N, steps))


def _replay_on_the_step_kernel(env, st0, ep0, d, D):
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


@pytest.mark.parametrize("which,N,T", [("acrobot", 50, 37), ("acrobot", 4096, 500), ("acrobot", 17, 2),
                                       ("mountaincar", 50, 37), ("mountaincar", 4096, 200), ("mountaincar", 17, 2)])
def test_chain_rollout_equals_the_step_kernel_bit_for_bit(which, N, T):
    """Two consecutive fused rollouts on the chain kernel; before each, env_state / ep_stats are copied, and the rollout's
    recorded actions are replayed through the stand-alone step kernel from the copy.  Observations, rewards, masks and
    the final env_state / ep_stats must be IDENTICAL: this pins Acrobot's speculative step (three candidates and a reset
    record per row on the env service, the sampled one selected by wave 0) and MountainCar's pre / post split,
    independently of how the towers round.  (17, 2): fewer envs than a tile, fewer steps than the rings are deep."""
    D = ENVS[which][1]
    cfg, env, net, trainer, buf, agent = _build(which, N, T, seed=4)
    drv = _driver(cfg, env, trainer, buf, agent)
    assert drv.fused
    drv.reset_and_buffer_init()
    dones = 0
    for k in range(2):
        st0, ep0 = env.env_state.clone(), env.ep_stats.clone()
        drv.actor_rollout()
        d = buf.data
        o, r, dn, st, ep = _replay_on_the_step_kernel(env, st0, ep0, d, D)
        assert np.array_equal(d.policy_obs[1:, :, 0].cpu().numpy(), o), k
        assert np.array_equal(d.rewards[:, :, 0, 0].cpu().numpy(), r), k
        assert np.array_equal(d.masks[1:, :, 0, 0].cpu().numpy(), (dn == 0).astype(np.float32)), k
        assert np.array_equal(env.env_state.cpu().numpy(), st), k
        assert np.array_equal(env.ep_stats.cpu().numpy(), ep), k
        dones += int(dn.sum())
        drv.compute_returns()
        buf.data.after_update()
    print("%s %d x %d: %d dones over two rollouts" % (which, N, T, dones))


@pytest.mark.parametrize("which", ["acrobot", "mountaincar"])
def test_chain_rollout_equals_the_step_kernel_from_near_terminal_states(which):
    """As above, 4096 x 64, from start states next to the terminal set (Acrobot: th1 in [1.8, 2.4], |th2| <= 0.3, |dth|
    <= 1; MountainCar: p in [0.3, 0.55], v in [-0.02, 0.05]): the random initial policy terminates there often, so the
    chain kernel's terminal branches - Acrobot's terminal flags and the reset record selected on termination,
    MountainCar's goal test - are compared with the stand-alone kernel bit for bit as well."""
    N, T = 4096, 64
    D = ENVS[which][1]
    cfg, env, net, trainer, buf, agent = _build(which, N, T, seed=6)
    drv = _driver(cfg, env, trainer, buf, agent)
    assert drv.fused
    drv.reset_and_buffer_init()
    rs = np.random.RandomState(1)
    st = env.env_state.cpu().numpy()
    if which == "acrobot":
        st[:, :4] = np.stack([rs.uniform(1.8, 2.4, N), rs.uniform(-0.3, 0.3, N), rs.uniform(-1, 1, N),
                              rs.uniform(-1, 1, N)], axis=-1)
        obs = cc.acrobot_obs_f32(st[:, :4])
    else:
        st[:, :2] = np.stack([rs.uniform(0.3, 0.55, N), rs.uniform(-0.02, 0.05, N)], axis=-1)
        obs = st[:, :2].copy()
    env.env_state.copy_(torch.from_numpy(st))
    buf.data.policy_obs[0, :, 0].copy_(torch.from_numpy(obs))
    if buf.data.critic_obs is not buf.data.policy_obs:
        buf.data.critic_obs[0, :, 0].copy_(torch.from_numpy(obs))
    st0, ep0 = env.env_state.clone(), env.ep_stats.clone()
    drv.actor_rollout()
    d = buf.data
    o, r, dn, stf, ep = _replay_on_the_step_kernel(env, st0, ep0, d, D)
    assert np.array_equal(d.policy_obs[1:, :, 0].cpu().numpy(), o)
    assert np.array_equal(d.rewards[:, :, 0, 0].cpu().numpy(), r)
    assert np.array_equal(d.masks[1:, :, 0, 0].cpu().numpy(), (dn == 0).astype(np.float32))
    assert np.array_equal(env.env_state.cpu().numpy(), stf)
    assert np.array_equal(env.ep_stats.cpu().numpy(), ep)
    print("%s near-terminal: %d terminations in %d x %d" % (which, int(dn.sum()), N, T))
    assert dn.sum() >= N // 8


@pytest.mark.parametrize("which,T", [("acrobot", 500), ("mountaincar", 200)])
def test_chain_rollout_teacher_forced_vs_oracle_towers(which, T):
    """4096 x T on the chain kernel, every 8th step: values against the oracle critic, and the log-probability of the
    action the kernel took against the oracle policy's log-softmax on the kernel's own observations; the action itself
    against the oracle's inverse-CDF sample with the same Philox uniform wherever the uniform is not within 1e-4 of a
    class boundary."""
    N = 4096
    D = ENVS[which][1]
    cfg, env, net, trainer, buf, agent = _build(which, N, T, seed=5)
    drv = _driver(cfg, env, trainer, buf, agent)
    assert drv.fused
    mod = net.module
    step0 = int(mod.rng_step)
    drv.reset_and_buffer_init()
    drv.actor_rollout()
    d = buf.data
    pspec, cspec = po.TowerSpec(D, 3, po.HEAD_CATEGORICAL), po.TowerSpec(D, 1, po.HEAD_VALUE)
    tp, tc = mod.models["policy"].theta.cpu(), mod.models["critic"].theta.cpu()
    obs = d.policy_obs.cpu().numpy()
    n = np.arange(N, dtype=np.uint32)
    flips = 0
    for t in range(0, T, 8):
        x, _, _, _ = px.philox4x32_10(mod.act_seed, n, 0, step0 + t, 0)
        u = px.u01(x)
        v, a, _ = po.get_actions(pspec, tp, cspec, tc, obs[t, :, 0], obs[t, :, 0], None, False, u)
        np.testing.assert_allclose(d.value_preds[t, :, 0].cpu().numpy(), v, rtol=1e-4, atol=1e-5, err_msg="t=%d" % t)
        with torch.no_grad():
            lg = torch.log_softmax(po.tower_forward(pspec, tp, torch.from_numpy(obs[t, :, 0])), dim=-1).numpy()
        act = d.actions[t, :, 0, 0].cpu().numpy().astype(np.int64)
        np.testing.assert_allclose(d.action_log_probs[t, :, 0, 0].cpu().numpy(), lg[np.arange(N), act], rtol=1e-4,
                                   atol=1e-5, err_msg="t=%d" % t)
        cdf = np.cumsum(np.exp(lg), axis=-1)
        far = np.min(np.abs(cdf[:, :2] - u[:, None]), axis=-1) > 1e-4
        assert np.array_equal(act[far], a[far, 0].astype(np.int64)), t
        flips += int((act[~far] != a[~far, 0]).sum())
    print("%s: %d sampled actions within 1e-4 of a class boundary differ" % (which, flips))


@pytest.mark.parametrize("which,N,T", [("acrobot", 512, 500), ("mountaincar", 512, 200)])
def test_fused_against_stepwise_route(which, N, T):
    """The chain kernel (fused) and the stepwise route on the same seeds.  The env arithmetic of both routes is one code
    (the bit-exact test above), the towers round differently (the chain's head from LayerNorm-2 partials, its critic an
    fp16 two-term split): a sampled action flips only where the Philox uniform lies within rounding of a class boundary,
    and from there the env trajectories diverge - Acrobot chaotically, MountainCar slowly.  Measured on a MI355X at 512
    envs: the fraction of envs whose actions and masks are identical through step 50, 100, ... was 1.0 at every checkpoint
    for both envs (Acrobot through step 500, MountainCar through step 200) - no sampled action landed within rounding of
    a class boundary at this shape.  Required: >= 99 % through step 50 and >= 95 % through the whole rollout (a flip
    anywhere takes an Acrobot env off the identical set for good; 5 % allows ~25 of 512 envs to meet one)."""
    seed = 3
    out = {}
    for mode in ("fused", "stepwise"):
        cfg, env, net, trainer, buf, agent = _build(which, N, T, seed=seed)
        cfg.amd_rollout_mode = mode
        cfg.amd_use_graph = False
        drv = _driver(cfg, env, trainer, buf, agent)
        assert drv.fused == (mode == "fused")
        drv.reset_and_buffer_init()
        drv.actor_rollout()
        out[mode] = (buf.data.actions[:, :, 0, 0].cpu().numpy(), buf.data.masks[1:, :, 0, 0].cpu().numpy())
    (aa, ma), (ab, mb) = out["fused"], out["stepwise"]
    same = (aa == ab) & (ma == mb)
    first = same[:50].all(axis=0).mean()
    per50 = [float(same[:i].all(axis=0).mean()) for i in range(50, T + 1, 50)]
    print("%s: envs identical through step 50, 100, ...: %s" % (which, per50))
    assert first >= 0.99, first
    assert per50[-1] >= 0.95, per50


def test_mountaincar_scripted_policy_reaches_the_goal():
    """Push in the direction of the velocity (action 2 if v >= 0, else 0) through env.step: every one of 512 envs
    terminates before step 200, and ep_stats records the episode lengths (= -returns) the oracle predicts."""
    from openrl_amd.envs.common import make

    N, seed = 512, 9
    env = make("MountainCar-v0", env_num=N, seed=seed, device=DEV)
    env.reset(seed=seed)
    orc = cc.MountainCarEnvOracle(N, seed)
    length = np.zeros(N, np.int64)  # of the first episode
    n_fin, len_fin, start = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64)
    for t in range(1, 200):
        v = env.env_state[:, 1].cpu().numpy()
        a = np.where(v >= 0, 2, 0)
        _, _, d, _ = env.step(a.reshape(N, 1, 1))
        _, _, od, _ = orc.step(a.reshape(N, 1, 1))
        assert np.array_equal(d[:, 0], od[:, 0]), t
        dn = d[:, 0]
        length = np.where((length == 0) & dn, t, length)
        n_fin += dn
        len_fin += np.where(dn, t - start, 0)
        start = np.where(dn, t, start)
        if (length > 0).all():
            break
    assert (length > 0).all() and length.max() < 200, length.max()
    es = env.ep_stats.cpu().numpy()
    np.testing.assert_array_equal(es[:, 3], n_fin.astype(np.float32))
    np.testing.assert_array_equal(es[:, 2], -len_fin.astype(np.float32))  # reward -1 per step: return = -length
    print("scripted MountainCar episode lengths: min %d, mean %.1f, max %d" % (length.min(), length.mean(), length.max()))


@pytest.mark.parametrize("which", ["acrobot", "mountaincar"])
@pytest.mark.parametrize("argv", [["--hidden_size", "128"], ["--use_recurrent_policy", "true"]])
def test_general_and_recurrent_towers_train_stepwise_and_graph_replayed(which, argv):
    """Towers outside the fused instances roll out through the stepwise route: the first rollout eagerly, the second
    replayed from the captured hipGraph; two iterations train."""
    N, T = 32, 16
    cfg, env, net, trainer, buf, agent = _build(which, N, T, seed=1, argv=argv + ["--log_interval", "1000000"])
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
    assert set(torch.unique(d.actions).cpu().tolist()) <= {0.0, 1.0, 2.0}
    assert (d.rewards <= 0).all()
    for k, m in net.module.models.items():
        if th0[k] is not None:
            assert not torch.equal(th0[k], m.theta.detach())


@pytest.mark.parametrize("which", ["acrobot", "mountaincar"])
def test_lockstep_kernel_is_refused_with_a_message(which):
    from openrl_amd import _native as nat

    cfg, env, net, trainer, buf, agent = _build(which, 32, 8)
    cfg.amd_rollout_kernel = "lockstep"
    drv = _driver(cfg, env, trainer, buf, agent)
    drv.reset_and_buffer_init()
    with pytest.raises(nat.NativeError, match="lockstep"):
        drv.actor_rollout()
    # the next call (the chain kernel) still works
    cfg.amd_rollout_kernel = "chain"
    drv2 = _driver(cfg, env, trainer, buf, agent)
    drv2.reset_and_buffer_init()
    drv2.actor_rollout()
    assert torch.isfinite(buf.data.value_preds).all() and (buf.data.rewards <= 0).all()


LEARN_N, LEARN_T, LEARN_ITERS, LEARN_SEEDS = 64, 500, 25, (0, 1, 2)
LEARN_FLOOR = 260.0


def _gain(curve):
    return float(np.mean(curve[-3:]) - np.mean(curve[:3]))


def _episode_returns(rew, done, acc):
    """Mean return of the episodes that finished in this rollout; ``acc`` carries the running returns across rollouts."""
    fin = []
    for t in range(rew.shape[0]):
        acc += rew[t]
        fin.extend(acc[done[t]].tolist())
        acc[done[t]] = 0.0
    return float(np.mean(fin)) if fin else float(-rew.shape[0])


def _learn_engine(seed):
    cfg, env, net, trainer, buf, agent = _build("acrobot", LEARN_N, LEARN_T, seed=seed, argv=["--log_interval", "1000000"])
    cfg.num_env_steps = LEARN_N * LEARN_T * LEARN_ITERS
    drv = _driver(cfg, env, trainer, buf, agent)
    assert drv.fused
    drv.reset_and_buffer_init()
    acc, curve = np.zeros(LEARN_N), []
    for i in range(LEARN_ITERS):
        drv.episode = i
        st0, ep0 = env.env_state.clone(), env.ep_stats.clone()
        drv._inner_loop()
        if i == LEARN_ITERS - 1:  # the trained policy terminates: its rollout replayed on the step kernel, bit for bit
            o, r, dn, st, ep = _replay_on_the_step_kernel(env, st0, ep0, buf.data, 6)
            assert np.array_equal(buf.data.policy_obs[1:, :, 0].cpu().numpy(), o)
            assert np.array_equal(buf.data.rewards[:, :, 0, 0].cpu().numpy(), r)
            assert np.array_equal(env.env_state.cpu().numpy(), st) and np.array_equal(env.ep_stats.cpu().numpy(), ep)
        rew = buf.data.rewards[:, :, 0, 0].cpu().numpy()
        done = buf.data.masks[1:, :, 0, 0].cpu().numpy() == 0  # (after_update keeps rows 1.. of this rollout)
        curve.append(_episode_returns(rew, done, acc))
    return curve


def _learn_port(seed):
    from oracle.cpu_trainer import CPUTrainer

    tr = CPUTrainer(LEARN_N, LEARN_T, obs_dim=6, n_actions=3, seed=seed, ppo_epoch=10, num_mini_batch=1, threads=8,
                    env=cc.AcrobotEnvOracle(LEARN_N, seed))
    acc, curve = np.zeros(LEARN_N), []
    for _ in range(LEARN_ITERS):
        tr.iterate()
        curve.append(_episode_returns(tr.buf.rewards[:, :, 0, 0], tr.buf.masks[1:, :, 0, 0] == 0, acc))
    return curve


def test_acrobot_learning_engine_vs_cpu_port():
    """Engine (fused chain rollout, default recipe) and the CPU port of the reference's maths on the same restated env,
    3 seeds, 64 envs x 500 steps x 25 iterations.  Score: the mean return of the episodes finished in the last 3
    iterations minus the first 3.  Engine median gain >= 0.85 x the port's, smallest engine gain >= LEARN_FLOOR.  A random
    policy hardly ever reaches the line: episodes are truncated at 500 steps, return -500.

    Measured on a MI355X (mean finished-episode return every 4th iteration, then the last):
        seed 0 engine -496 -399 -147 -112  -98 -93 -88 -88
               port   -498 -500 -186 -115  -97 -93 -87 -87
        seed 1 engine -500 -500 -491 -150 -106 -96 -88 -88
               port   -500 -500 -500 -160 -114 -94 -91 -91
        seed 2 engine -497 -199 -112 -102  -91 -87 -86 -86
               port   -498 -289 -120 -100  -94 -88 -88 -88
    gains: engine 410.8 / 406.0 / 374.9, port 410.6 / 408.8 / 404.0.  The floor (260) leaves ~30 % margin under the
    smallest engine gain.  The test took 71.5 s on the MI355X (engine and CPU port together).  The last iteration's
    rollout (a trained policy: ~5 terminations per env) is also replayed on the stand-alone step kernel and must match
    bit for bit.

    MountainCar-v0 gets no learning assertion: its reward is -1 on every step until the goal, and PPO at default settings
    often never reaches the goal by chance, so there is nothing to learn from."""
    eng = [_learn_engine(s) for s in LEARN_SEEDS]
    port = [_learn_port(s) for s in LEARN_SEEDS]
    ge, gp = [_gain(c) for c in eng], [_gain(c) for c in port]
    for s, ce, cp in zip(LEARN_SEEDS, eng, port):
        print("seed %d engine %s" % (s, [round(x) for x in ce[::4]] + [round(ce[-1])]))
        print("seed %d port   %s" % (s, [round(x) for x in cp[::4]] + [round(cp[-1])]))
    print("gains: engine %s port %s" % ([round(g, 1) for g in ge], [round(g, 1) for g in gp]))
    assert np.median(ge) >= 0.85 * np.median(gp), (ge, gp)
    assert min(ge) >= LEARN_FLOOR, (ge, gp)
