"""PPO update parity: the HIP engine replays the reference's ``PPOAlgorithm.train`` golden cases
(same initial weights, same buffer, same host permutation stream) and must land on the reference's
final weights / train_info / ValueNorm state within the stated fp32 tolerance.  Needs a MI355X."""
import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# fp32 tolerance stated for this path: the GPU sums gradients tile-by-tile in a different order than the
# CPU GEMMs and uses MFMA k-ordering; parameters move by lr=5e-4 per step so 5 updates stay well below.
THETA_RTOL, THETA_ATOL = 2e-3, 3e-5
INFO_RTOL, INFO_ATOL = 2e-4, 2e-5


def _assert_thetas(g, module):
    """First line: the bar on the UPDATE d_theta = theta_1 - theta_0 (cosine + 2 % of |d_ref| on >= 99 % of the
    entries, tests/helpers.py) - the claim that can fail; second line: the historical check on theta_1 itself."""
    for name, k0, k1 in (("policy", "theta_p0", "theta_p1"), ("critic", "theta_c0", "theta_c1")):
        got = module.models[name].theta.cpu().numpy()
        # + the per-block bar: every parameter block (W1 .. b3 / logstd) points the reference's way on its own
        H.assert_update_parity(g[k0], got, g[k1], name, blocks=H.blocks_of(module.models[name]))
        np.testing.assert_allclose(got, g[k1], rtol=THETA_RTOL, atol=THETA_ATOL)


def build_engine(g):
    from openrl_amd import spaces
    from openrl_amd.algorithms.ppo import PPOAlgorithm
    from openrl_amd.buffers.replay_data import ReplayData
    from openrl_amd.modules.ppo_module import PPOModule

    cfg = H.case_cfg(g)
    T, N, A, D = g["buf_policy_obs"].shape[0] - 1, g["buf_policy_obs"].shape[1], 1, g["buf_policy_obs"].shape[-1]
    cfg.episode_length, cfg.n_rollout_threads, cfg.num_agents = T, N, A
    cfg.rnn_hidden_size = cfg.hidden_size
    obs_space = spaces.Box(-np.inf, np.inf, (D,))
    if "buf_action_masks" in g:
        act_space = spaces.Discrete(g["buf_action_masks"].shape[-1])
    else:
        act_space = spaces.Box(-1, 1, (g["buf_actions"].shape[-1],))
    torch.manual_seed(0)
    module = PPOModule(cfg, obs_space, obs_space, act_space, device=DEV, rank=0, world_size=1)
    module.models["policy"].theta.copy_(torch.tensor(g["theta_p0"]))
    module.models["critic"].theta.copy_(torch.tensor(g["theta_c0"]))
    buf = ReplayData(cfg, A, obs_space, act_space, device=DEV)
    for f in ("policy_obs", "actions", "action_log_probs", "value_preds", "returns", "rewards", "masks", "bad_masks",
              "active_masks", "action_masks"):
        if "buf_" + f in g:
            getattr(buf, f).copy_(torch.tensor(g["buf_" + f]))
    algo = PPOAlgorithm(cfg, module, agent_num=A, device=DEV)
    return cfg, module, buf, algo


@pytest.mark.parametrize("case", H.TRAIN_CASES)
def test_train_matches_reference_golden(case):
    g = H.load_golden(case)
    cfg, module, buf, algo = build_engine(g)
    torch.manual_seed(int(g["perm_seed"]))
    algo.prep_training()
    info = algo.train(buf)
    # minibatch order: bit-exact with the reference's BatchSampler(SubsetRandomSampler) stream
    r = H.oracle_replay(g)
    assert len(algo.last_indices) == len(r["used"])
    for got, want in zip(algo.last_indices, r["used"]):
        assert np.array_equal(got.cpu().numpy(), want)
    # advantages (K7) vs oracle
    np.testing.assert_allclose(buf.advantages.cpu().numpy(), r["adv"], rtol=2e-5, atol=2e-5)
    got = np.array([info[k] for k in ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm",
                                      "critic_grad_norm", "ratio")])
    np.testing.assert_allclose(got, g["train_info"], rtol=INFO_RTOL, atol=INFO_ATOL)
    _assert_thetas(g, module)
    if "vn_state1" in g:
        np.testing.assert_allclose(module.get_critic_value_normalizer().state.cpu().numpy(), g["vn_state1"],
                                   rtol=1e-5)


def _assert_golden_outputs(g, module, info):
    got = np.array([info[k] for k in ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm",
                                      "critic_grad_norm", "ratio")])
    np.testing.assert_allclose(got, g["train_info"], rtol=INFO_RTOL, atol=INFO_ATOL)
    _assert_thetas(g, module)
    if "vn_state1" in g:
        np.testing.assert_allclose(module.get_critic_value_normalizer().state.cpu().numpy(), g["vn_state1"],
                                   rtol=1e-5)


@pytest.mark.parametrize("perm_mode", ["device", "identity"])
@pytest.mark.parametrize("case", [c for c in H.TRAIN_CASES if "--num_mini_batch 1" in str(H.load_golden(c)["argv"])])
def test_device_and_identity_permutation_land_on_the_reference_golden(case, perm_mode):
    """What bench.py runs (``amd_perm_mode=device``) against the REFERENCE's outputs: with one minibatch per epoch the
    permutation only changes the fp32 summation order, so the reference's final weights / train_info / ValueNorm
    state (reached with its own torch.randperm stream) must be hit at the same tolerances as in reference mode."""
    g = H.load_golden(case)
    cfg, module, buf, algo = build_engine(g)
    assert cfg.num_mini_batch == 1
    algo.perm_mode = perm_mode
    algo.prep_training()
    info = algo.train(buf)
    _assert_golden_outputs(g, module, info)


@pytest.mark.parametrize("case", ["train_discrete", "train_gaussian"])
def test_update_parity_bar_rejects_a_short_or_partial_engine_update(case):
    """Negative controls of the d_theta bar ON THE ENGINE: the same golden case with the last epoch skipped, and the
    engine's own full update with one layer's block left at theta_0 (= that layer's gradient dropped), must both be
    refused - while the historical assert_allclose on theta_1 accepts the short run on most entries."""
    g = H.load_golden(case)
    cfg, module, buf, algo = build_engine(g)
    torch.manual_seed(int(g["perm_seed"]))
    algo.prep_training()
    algo.train(buf)
    _assert_thetas(g, module)
    full_p = module.models["policy"].theta.cpu().numpy()
    pspec, _ = H.case_specs(g)
    for block in ("W1", "W2", "b2", "W3"):
        H.assert_update_parity_rejects(g["theta_p0"], H.without_block_update(g["theta_p0"], full_p, pspec, block),
                                       g["theta_p1"], "policy without d" + block)
    # a bug confined to a tiny block (b3: 1 - 6 entries; logstd) fits the global bar's 1 % exception budget: the per-block bar
    # (tests/helpers.py::assert_block_update_parity) has to refuse it, on both towers
    for name, k0, k1, spec in (("policy", "theta_p0", "theta_p1", pspec), ("critic", "theta_c0", "theta_c1", H.case_specs(g)[1])):
        full = module.models[name].theta.cpu().numpy()
        blocks = H.tower_blocks(spec)
        for block in ("b3", "logstd"):
            if block in blocks:
                H.assert_update_parity_rejects(g[k0], H.without_block_update(g[k0], full, spec, block), g[k1],
                                               "%s without d%s" % (name, block), blocks=blocks)
    cfg2, module2, buf2, algo2 = build_engine(g)
    algo2.ppo_epoch -= 1
    torch.manual_seed(int(g["perm_seed"]))
    algo2.prep_training()
    algo2.train(buf2)
    for name, k0, k1 in (("policy", "theta_p0", "theta_p1"), ("critic", "theta_c0", "theta_c1")):
        H.assert_update_parity_rejects(g[k0], module2.models[name].theta.cpu().numpy(), g[k1],
                                       name + ", last epoch skipped")


@pytest.mark.parametrize("perm_mode", ["device", "identity", "reference"])
def test_full_size_update_matches_reference_golden(perm_mode):
    """BASELINE.json configs[1] at FULL size - 4096 envs x 128 steps = 524 288 rows, obs 4, Discrete(2), ppo_epoch 10,
    one minibatch, ValueNorm on: 256 workgroups x 128 tiles per tower launch, the partial-reduce depth and the
    ``gae_max_partials`` regime of the bench.  The buffer is regenerated from the seed (oracle/fixtures.py); the
    expected outputs are the REAL reference's ``compute_returns`` + ``PPOAlgorithm.train`` (oracle/gen_golden.py,
    case train_cfg2_full; reference algorithms/ppo.py:383-458, buffers/replay_data.py:320-423,553-646)."""
    g = H.load_golden("train_cfg2_full")
    cfg, module, buf, algo = _cfg2_full_engine(g)
    algo.perm_mode = perm_mode
    torch.manual_seed(int(g["perm_seed"]))
    algo.prep_training()
    info = algo.train(buf)
    _assert_golden_outputs(g, module, info)


def _cfg2_full_engine(g):
    from openrl_amd import spaces
    from openrl_amd.algorithms.ppo import PPOAlgorithm
    from openrl_amd.buffers.replay_data import ReplayData
    from openrl_amd.modules.ppo_module import PPOModule
    from oracle.fixtures import synth_update_buffer

    N, T, D, n_act, seed = (int(x) for x in g["shape"])
    cfg = H.case_cfg(g)
    cfg.episode_length, cfg.n_rollout_threads, cfg.num_agents, cfg.rnn_hidden_size = T, N, 1, cfg.hidden_size
    obs_space, act_space = spaces.Box(-np.inf, np.inf, (D,)), spaces.Discrete(n_act)
    torch.manual_seed(0)
    module = PPOModule(cfg, obs_space, obs_space, act_space, device=DEV, rank=0, world_size=1)
    module.models["policy"].theta.copy_(torch.tensor(g["theta_p0"]))
    module.models["critic"].theta.copy_(torch.tensor(g["theta_c0"]))
    buf = ReplayData(cfg, 1, obs_space, act_space, device=DEV)
    src = synth_update_buffer(seed, N, T, D, n_act)
    for f in ("policy_obs", "rewards", "value_preds", "masks", "active_masks", "bad_masks", "actions",
              "action_log_probs", "action_masks"):
        getattr(buf, f).copy_(torch.tensor(src[f]))
    buf.compute_returns(torch.tensor(src["next_value"]), module.get_critic_value_normalizer())
    ret = buf.returns.cpu().numpy()
    probe = np.array([ret[t, n, 0, 0] for t, n in g["returns_probe_idx"]])
    np.testing.assert_allclose(probe, g["returns_probe"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(ret[:-1].astype(np.float64).sum(), float(g["returns_sum"]), rtol=1e-6)
    algo = PPOAlgorithm(cfg, module, agent_num=1, device=DEV)
    return cfg, module, buf, algo


@pytest.mark.parametrize("case", H.TRAIN_CASES)
def test_single_update_gradients_vs_oracle(case):
    """One minibatch: clipped parameter gradients of both towers against torch autograd on the oracle."""
    single_update_vs_oracle(H.load_golden(case))


def single_update_vs_oracle(g, grad_atol=2e-5, info_rtol=INFO_RTOL, info_atol=INFO_ATOL, theta_atol=1e-5):
    """(also driven by tests/test_layernorm_adversarial_gpu.py on golden cases with shifted initial weights; grad_atol is
    relative to the largest gradient entry of the tower)"""
    cfg, module, buf, algo = build_engine(g)
    r0 = H.oracle_replay(g)  # for cfg/hp/specs only
    hp, pspec, cspec = r0["hp"], r0["pspec"], r0["cspec"]
    # oracle single update on the full batch in identity order
    ptheta, ctheta = torch.tensor(g["theta_p0"]).clone(), torch.tensor(g["theta_c0"]).clone()
    padam = po.AdamOracle(ptheta.numel(), cfg.lr, cfg.opti_eps, cfg.weight_decay)
    cadam = po.AdamOracle(ctheta.numel(), cfg.critic_lr, cfg.opti_eps, cfg.weight_decay)
    vn = po.ValueNormOracle() if cfg.use_valuenorm else None
    b = H.case_buffer(g)
    adv = po.advantages(b["returns"], b["value_preds"], b["active_masks"], vn if hp.use_valuenorm else None,
                        hp.use_adv_normalize)
    fr = po.flat_rows
    sample = (fr(b["critic_obs"][:-1]), fr(b["policy_obs"][:-1]), fr(b["actions"]), fr(b["value_preds"][:-1]),
              fr(b["returns"][:-1]), fr(b["active_masks"][:-1]), fr(b["action_log_probs"]), adv.reshape(-1, 1),
              None if b["action_masks"] is None else fr(b["action_masks"][:-1]))
    info_o, gp, gc = po.ppo_update(hp, pspec, ptheta, cspec, ctheta, padam, cadam, vn, sample)
    # engine: same thing through the C ABI
    algo._advantages_and_records(buf)
    M = adv.size
    algo._info.zero_()
    algo._update_minibatch(buf, None, M, True)
    got_p = module.models["policy"].grad.cpu().numpy()
    got_c = module.models["critic"].grad.cpu().numpy()
    scale_p, scale_c = np.abs(gp).max(), np.abs(gc).max()
    np.testing.assert_allclose(got_p, gp, rtol=1e-3, atol=grad_atol * scale_p + 1e-7)
    np.testing.assert_allclose(got_c, gc, rtol=1e-3, atol=grad_atol * scale_c + 1e-7)
    got_info = algo._info[:6].cpu().numpy()
    want = np.array([info_o[k] for k in ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm",
                                         "critic_grad_norm", "ratio")])
    np.testing.assert_allclose(got_info, want, rtol=info_rtol, atol=info_atol)
    np.testing.assert_allclose(module.models["policy"].theta.cpu().numpy(), ptheta.numpy(), rtol=1e-3, atol=theta_atol)
    np.testing.assert_allclose(module.models["critic"].theta.cpu().numpy(), ctheta.numpy(), rtol=1e-3, atol=theta_atol)


def test_device_permutation_mode_trains_and_is_deterministic():
    g = H.load_golden("train_discrete")
    outs = []
    for _ in range(2):
        cfg, module, buf, algo = build_engine(g)
        algo.perm_mode = "device"
        info = algo.train(buf)
        outs.append((module.models["policy"].theta.cpu().numpy().copy(), info))
        idx = torch.cat(algo.last_indices[:cfg.num_mini_batch]).cpu().numpy()
        assert len(set(idx.tolist())) == idx.size  # a permutation, not a resample
    assert np.array_equal(outs[0][0], outs[1][0]), "same seed must give bit-identical weights"
    assert np.isfinite(list(outs[0][1].values())).all()


@pytest.mark.parametrize("case", ["train_discrete", "train_discrete_masks"])
def test_next_epoch_permutation_in_the_apply_launch_changes_nothing(case):
    """orl_ppo_apply_perm: epoch e+1's permutation (+ ValueNorm.update when the minibatch is the whole batch) produced
    by idle workgroups of epoch e's optimiser step == the stand-alone launches, bit for bit."""
    g = H.load_golden(case)
    outs = []
    for fuse in (True, False):
        cfg, module, buf, algo = build_engine(g)
        algo.perm_mode, algo.fuse_next_perm = "device", fuse
        algo.train(buf)
        vn = module.get_critic_value_normalizer()
        outs.append((module.models["policy"].theta.clone(), module.models["critic"].theta.clone(),
                     None if vn is None else vn.state.clone(), [i.clone() for i in algo.last_indices]))
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert (a[2] is None and b[2] is None) or torch.equal(a[2], b[2])
    assert len(a[3]) == len(b[3]) and all(torch.equal(x, y) for x, y in zip(a[3], b[3]))


@pytest.mark.parametrize("one_launch", ["step", H.experimental("fused")])
@pytest.mark.parametrize("turn_on", [True, False])
@pytest.mark.parametrize("perm_mode", ["device", "reference"])
@pytest.mark.parametrize("case", ["train_discrete", "train_discrete_masks", "train_gaussian", "train_cfg2_full"])
def test_one_launch_optimiser_step_equals_the_two_launch_one_bit_for_bit(case, perm_mode, turn_on, one_launch):
    """The one-launch optimiser steps == orl_ppo_reduce_pair + orl_ppo_apply(_perm): weights, Adam moments, sums, train_info,
    ValueNorm state and every epoch's indices identical; the ticket words are back at zero after every call.
    ``step`` = orl_ppo_step (round 6: two designated optimiser workgroups wait for the write-through column sums behind a
    ticket word - same time as two launches, so not the default); ``fused`` = orl_ppo_reduce_apply (round 5's ticketed form behind cache fences, a
    comparison kernel)."""
    g = H.load_golden(case)
    outs = []
    for step in (one_launch, "two_launch"):
        cfg, module, buf, algo = _cfg2_full_engine(g) if case == "train_cfg2_full" else build_engine(g)
        assert algo._optim_step == "two_launch" and not algo._fused_step  # two launches are the default (equal time, simpler)
        algo._optim_step, algo._fused_step = step, step != "two_launch"
        algo.perm_mode = perm_mode
        info = [dict(algo.train(buf, turn_on=turn_on)) for _ in range(2)]  # the second call starts from a used ticket array
        assert algo._sync_ctr.cpu().tolist() == [0, 0, 0, 0]
        vn = module.get_critic_value_normalizer()
        opt = module.optimizers
        outs.append(dict(p=module.models["policy"].theta.clone(), c=module.models["critic"].theta.clone(),
                         pm=opt["policy"].exp_avg.clone(), pv=opt["policy"].exp_avg_sq.clone(),
                         cm=opt["critic"].exp_avg.clone(), cv=opt["critic"].exp_avg_sq.clone(), sums=algo._sums.clone(),
                         vn=None if vn is None else vn.state.clone(), idx=[i.clone() for i in algo.last_indices],
                         info=info))
    a, b = outs
    for k in ("p", "c", "pm", "pv", "cm", "cv", "sums"):
        assert torch.equal(a[k], b[k]), k
    assert (a["vn"] is None and b["vn"] is None) or torch.equal(a["vn"], b["vn"])
    assert len(a["idx"]) == len(b["idx"]) and all(torch.equal(x, y) for x, y in zip(a["idx"], b["idx"]))
    assert a["info"] == b["info"]


@pytest.mark.parametrize("case", ["train_discrete", "train_gaussian"])
def test_turn_on_false_updates_only_the_critic(case):
    """PPOAlgorithm.train(buffer, turn_on=False) (ppo.py:226-236: the policy loss is not in the loss list): the policy
    parameters and its Adam state do not move, the critic gets exactly the update it gets with turn_on=True."""
    g = H.load_golden(case)
    res = []
    for turn_on in (True, False):
        cfg, module, buf, algo = build_engine(g)
        algo.perm_mode = "device"
        p0 = module.models["policy"].theta.clone()
        info = algo.train(buf, turn_on=turn_on)
        res.append((module.models["policy"].theta.clone(), module.models["critic"].theta.clone(), dict(info), p0,
                    module.optimizers["policy"].step_count))
    on, off = res
    assert torch.equal(off[0], off[3]) and off[4] == 0 and not torch.equal(on[0], on[3])
    assert torch.equal(on[1], off[1])  # the critic tower never sees the policy
    assert off[2]["actor_grad_norm"] == 0.0 and np.isfinite(list(off[2].values())).all()
    assert off[2]["value_loss"] == on[2]["value_loss"]


def _random_case(D, act_space_kind, n_act, N, T, seed, masks=False):
    """Synthetic buffer at an arbitrary shape: one full-batch update, engine vs oracle autograd."""
    from openrl_amd import spaces
    from openrl_amd.algorithms.ppo import PPOAlgorithm
    from openrl_amd.buffers.replay_data import ReplayData
    from openrl_amd.configs.config import default_cfg
    from openrl_amd.modules.ppo_module import PPOModule

    rs = np.random.RandomState(seed)
    cfg = default_cfg(["--seed", str(seed), "--episode_length", str(T), "--ppo_epoch", "1"])
    cfg.n_rollout_threads, cfg.num_agents, cfg.rnn_hidden_size = N, 1, cfg.hidden_size
    obs_space = spaces.Box(-np.inf, np.inf, (D,))
    act_space = spaces.Discrete(n_act) if act_space_kind == "discrete" else spaces.Box(-1, 1, (n_act,))
    torch.manual_seed(seed)
    module = PPOModule(cfg, obs_space, obs_space, act_space, device=DEV, rank=0, world_size=1)
    buf = ReplayData(cfg, 1, obs_space, act_space, device=DEV)
    a_w = 1 if act_space_kind == "discrete" else n_act
    host = dict(policy_obs=rs.randn(T + 1, N, 1, D).astype(np.float32),
                rewards=rs.rand(T, N, 1, 1).astype(np.float32),
                value_preds=(0.3 * rs.randn(T + 1, N, 1, 1)).astype(np.float32),
                masks=(rs.rand(T + 1, N, 1, 1) > 0.05).astype(np.float32),
                active_masks=(rs.rand(T + 1, N, 1, 1) > 0.1).astype(np.float32))
    if act_space_kind == "discrete":
        host["actions"] = rs.randint(0, n_act, (T, N, 1, 1)).astype(np.float32)
        host["action_log_probs"] = np.log(np.full((T, N, 1, 1), 1.0 / n_act, np.float32)) + 0.05 * rs.randn(T, N, 1, 1).astype(np.float32)
        if masks:
            am = (rs.rand(T + 1, N, 1, n_act) > 0.3).astype(np.float32)
            am[np.arange(T)[:, None], np.arange(N)[None, :], 0, host["actions"][..., 0, 0].astype(int)] = 1.0
            host["action_masks"] = am
    else:
        host["actions"] = rs.randn(T, N, 1, n_act).astype(np.float32)
        host["action_log_probs"] = (-0.5 * host["actions"] ** 2 - 0.9189385 + 0.05 * rs.randn(T, N, 1, n_act)).astype(np.float32)
    for k, v in host.items():
        getattr(buf, k).copy_(torch.tensor(v))
    host["critic_obs"] = host["policy_obs"]
    host.setdefault("action_masks", None if act_space_kind != "discrete" else np.ones((T + 1, N, 1, n_act), np.float32))
    buf.compute_returns(torch.tensor(0.3 * rs.randn(N, 1, 1).astype(np.float32)), module.get_critic_value_normalizer())
    host["returns"], host["value_preds"] = buf.returns.cpu().numpy(), buf.value_preds.cpu().numpy()
    return cfg, module, buf, PPOAlgorithm(cfg, module, agent_num=1, device=DEV), host, a_w


@pytest.mark.parametrize("D,kind,n_act,N,T,masks", [
    (17, "gaussian", 6, 64, 25, False),    # config 3 shape: HalfCheetah obs 17, Box(6)
    (18, "discrete", 9, 64, 25, True),     # config 5 shape: tictactoe obs 18, Discrete(9) + action masks
    (18, "discrete", 5, 48, 25, False),    # MPE simple_spread policy obs 18, Discrete(5) (feed-forward part)
    (4, "discrete", 2, 1024, 32, False),   # config 2 shape, 2048 tiles
    (3, "discrete", 3, 7, 5, False),       # ragged: 35 rows, obs not a multiple of 4
    (64, "discrete", 16, 40, 9, True),     # the widest tower the kernels admit: obs 64, 16 classes, masks
    (33, "gaussian", 16, 20, 7, False),    # obs 33: two 16-column dW1 blocks + a 1-column remainder; Box(16)
    (20, "discrete", 4, 33, 6, False),     # obs 20: one dW1 block + a 4-column remainder; narrow head at NO = 8
    (54, "gaussian", 1, 18, 5, False),     # MPE critic-sized obs with a one-dimensional Gaussian head
])
def test_single_update_at_baseline_shapes_vs_oracle(D, kind, n_act, N, T, masks):
    cfg, module, buf, algo, host, a_w = _random_case(D, kind, n_act, N, T, seed=D + n_act, masks=masks)
    hp = po.hyper_from_cfg(cfg)
    head = po.HEAD_CATEGORICAL if kind == "discrete" else po.HEAD_GAUSSIAN
    pspec, cspec = po.TowerSpec(D, n_act, head), po.TowerSpec(D, 1, po.HEAD_VALUE)
    ptheta, ctheta = module.models["policy"].theta.cpu().clone(), module.models["critic"].theta.cpu().clone()
    padam, cadam = po.AdamOracle(ptheta.numel(), cfg.lr), po.AdamOracle(ctheta.numel(), cfg.critic_lr)
    vn = po.ValueNormOracle()
    adv = po.advantages(host["returns"], host["value_preds"], host["active_masks"], vn, False)
    fr = po.flat_rows
    sample = (fr(host["critic_obs"][:-1]), fr(host["policy_obs"][:-1]), fr(host["actions"]),
              fr(host["value_preds"][:-1]), fr(host["returns"][:-1]), fr(host["active_masks"][:-1]),
              fr(host["action_log_probs"]), adv.reshape(-1, 1),
              None if host["action_masks"] is None else fr(host["action_masks"][:-1]))
    info_o, gp, gc = po.ppo_update(hp, pspec, ptheta, cspec, ctheta, padam, cadam, vn, sample)
    algo._advantages_and_records(buf)
    np.testing.assert_allclose(buf.advantages.cpu().numpy(), adv, rtol=5e-5, atol=5e-5)
    algo._info.zero_()
    algo._update_minibatch(buf, None, adv.size, True)
    got_p, got_c = module.models["policy"].grad.cpu().numpy(), module.models["critic"].grad.cpu().numpy()
    np.testing.assert_allclose(got_p, gp, rtol=2e-3, atol=3e-5 * np.abs(gp).max() + 1e-7)
    np.testing.assert_allclose(got_c, gc, rtol=2e-3, atol=3e-5 * np.abs(gc).max() + 1e-7)
    want = np.array([info_o[k] for k in ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm",
                                         "critic_grad_norm", "ratio")])
    np.testing.assert_allclose(algo._info[:6].cpu().numpy(), want, rtol=3e-4, atol=3e-5)


def _full_general_engine(g, perm_mode, gemm=None):
    """Engine + buffer of a ``train_cfg{3,4,5}_full`` case (inputs regenerated from the seed, oracle/fixtures.py);
    ``compute_returns`` has run and its probes were checked against the reference's."""
    from openrl_amd import spaces
    from openrl_amd.algorithms.ppo import PPOAlgorithm
    from openrl_amd.buffers.replay_data import ReplayData
    from openrl_amd.modules.ppo_module import PPOModule
    from oracle.fixtures import synth_update_buffer_general

    N, T, Dp, Dc, n_act, A, seed, legal, recurrent = (int(x) for x in g["shape"])
    kind = str(g["kind"])
    cfg = H.case_cfg(g)
    cfg.episode_length, cfg.n_rollout_threads, cfg.num_agents, cfg.rnn_hidden_size = T, N, A, cfg.hidden_size
    if gemm is not None:  # the update kernels' GEMM path: amd_tower_gemm (split | fp32 | split_two_image) for the
        if gemm in ("split", "fp32", "split_two_image"):  # feed-forward pair, amd_rnn_gemm (fp32 | split | split_w4) for the
            cfg.amd_tower_gemm = gemm                      # recurrent row kernel
        if gemm in ("split", "fp32", "split_w4", "fp32_recompute"):
            cfg.amd_rnn_gemm = gemm
    box = lambda d: spaces.Box(-np.inf, np.inf, (d,))
    obs_space = box(Dp) if Dp == Dc else spaces.Dict({"policy": box(Dp), "critic": box(Dc)})
    act_space = spaces.Discrete(n_act) if kind == "discrete" else spaces.Box(-1, 1, (n_act,))
    torch.manual_seed(0)
    module = PPOModule(cfg, obs_space, obs_space, act_space, device=DEV, rank=0, world_size=1)
    module.models["policy"].theta.copy_(torch.tensor(g["theta_p0"]))
    module.models["critic"].theta.copy_(torch.tensor(g["theta_c0"]))
    buf = ReplayData(cfg, A, obs_space, act_space, device=DEV)
    src = synth_update_buffer_general(seed, N, T, Dp, Dc, kind, n_act, A, bool(legal), cfg.hidden_size if recurrent else 0)
    for f in ("policy_obs", "critic_obs", "rewards", "value_preds", "masks", "active_masks", "bad_masks", "actions",
              "action_log_probs", "action_masks", "rnn_states", "rnn_states_critic"):
        if f in src and getattr(buf, f, None) is not None and (f != "critic_obs" or Dp != Dc):
            getattr(buf, f).copy_(torch.tensor(src[f]))
    buf.compute_returns(torch.tensor(src["next_value"]), module.get_critic_value_normalizer())
    ret = buf.returns.cpu().numpy()
    probe = np.array([ret[t, n, a, 0] for t, n, a in g["returns_probe_idx"]])
    np.testing.assert_allclose(probe, g["returns_probe"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(ret[:-1].astype(np.float64).sum(), float(g["returns_sum"]), rtol=1e-6)
    algo = PPOAlgorithm(cfg, module, agent_num=A, device=DEV)
    algo.perm_mode = perm_mode
    return cfg, module, buf, algo


@pytest.mark.parametrize("perm_mode,gemm", [("device", "split"), ("identity", "split"), ("reference", "split"),
                                            H.experimental("device", "split_two_image"), H.experimental("device", "fp32")])
@pytest.mark.parametrize("case,branch", [("train_cfg3_full", "uneven_split"), ("train_cfg5_full", "back_to_back")])
def test_full_size_update_other_baseline_shapes_match_reference_golden(case, branch, perm_mode, gemm):
    """BASELINE.json configs[2] (1024 x 200 rows, obs 17, Box(6)) and configs[4] (4096 x 200, obs 18, Discrete(9) with
    random legal-move masks) at FULL size against the REAL reference's ``compute_returns`` + ``PPOAlgorithm.train``
    (10 epochs; oracle/gen_golden.py::_train_case_full_general).  These are the batches where ``launch_pair_nd``
    (csrc/orl_ppo.hip) leaves its small-batch route: 12 800 tiles -> the UNEVEN side-by-side CU split of a wide head,
    51 200 tiles -> policy and critic workgroups BACK TO BACK; the test asserts from the workgroup counts the launch
    reports that the branch was really taken, with the wide-observation (ND = 1) pair kernel builds several tiles deep
    per wave."""
    from openrl_amd import ops

    # gemm: the default is round 4's full split through transposing reads of W2's image (+ dW1 on the bf16 MFMA);
    # split_two_image = round 3's variants (wgrad-only split at these widths), fp32 = every GEMM on the fp32 MFMA
    g = H.load_golden(case)
    cfg, module, buf, algo = _full_general_engine(g, perm_mode, gemm)
    grids, orig = [], ops.ppo_fwd_bwd

    def spy(*a, **k):
        r = orig(*a, **k)
        grids.append(r)
        return r

    ops.ppo_fwd_bwd = spy
    try:
        torch.manual_seed(int(g["perm_seed"]))
        algo.prep_training()
        info = algo.train(buf)
    finally:
        ops.ppo_fwd_bwd = orig
    mb = ops.ppo_max_blocks()
    assert len(grids) == cfg.ppo_epoch
    for gp, gc in grids:
        if branch == "uneven_split":
            assert gp + gc == mb and gp > gc, (gp, gc)
        else:
            assert gp == mb and gc == mb, (gp, gc)
    _assert_golden_outputs(g, module, info)


@pytest.mark.experiments  # the fp32-MFMA tower pair is a comparison kernel
def test_split_bf16_gemms_are_as_accurate_as_the_fp32_mfma_at_full_size():
    """The tower update's GEMMs as exact three-term bf16 splits (default) vs the fp32 MFMA (``amd_tower_gemm=fp32``,
    ``orl_ppo_hparams.reserved & 4``): one full-batch update at BASELINE configs[1]'s size (524 288 rows), clipped
    parameter gradients of both towers against a FLOAT64 autograd reference of the same loss.  The split build must be at
    least as close to fp64 as the fp32-MFMA build (up to 1.5x - both are dominated by the fp32 accumulation order), and
    the two builds must agree with each other to fp32 rounding of the sums."""
    from openrl_amd import spaces
    from openrl_amd.algorithms.ppo import PPOAlgorithm
    from openrl_amd.buffers.replay_data import ReplayData
    from openrl_amd.modules.ppo_module import PPOModule
    from oracle.fixtures import synth_update_buffer

    g = H.load_golden("train_cfg2_full")
    N, T, D, n_act, seed = (int(x) for x in g["shape"])
    src = synth_update_buffer(seed, N, T, D, n_act)
    grads = {}
    for mode in ("split", "fp32"):
        cfg = H.case_cfg(g)
        cfg.episode_length, cfg.n_rollout_threads, cfg.num_agents, cfg.rnn_hidden_size = T, N, 1, cfg.hidden_size
        cfg.amd_tower_gemm = mode
        obs_space, act_space = spaces.Box(-np.inf, np.inf, (D,)), spaces.Discrete(n_act)
        module = PPOModule(cfg, obs_space, obs_space, act_space, device=DEV, rank=0, world_size=1)
        module.models["policy"].theta.copy_(torch.tensor(g["theta_p0"]))
        module.models["critic"].theta.copy_(torch.tensor(g["theta_c0"]))
        buf = ReplayData(cfg, 1, obs_space, act_space, device=DEV)
        for f in ("policy_obs", "rewards", "value_preds", "masks", "active_masks", "bad_masks", "actions",
                  "action_log_probs", "action_masks"):
            getattr(buf, f).copy_(torch.tensor(src[f]))
        buf.compute_returns(torch.tensor(src["next_value"]), module.get_critic_value_normalizer())
        algo = PPOAlgorithm(cfg, module, agent_num=1, device=DEV)
        assert bool(algo.hp.reserved & 4) == (mode == "fp32")
        algo._advantages_and_records(buf)
        algo._info.zero_()
        vn = module.get_critic_value_normalizer()
        algo._update_minibatch(buf, None, N * T, True)  # ValueNorm.update(return_batch) runs inside, before the loss
        grads[mode] = (module.models["policy"].grad.double().cpu(), module.models["critic"].grad.double().cpu())
        if mode == "split":  # what the fp64 reference needs: the engine's own returns / advantages / ValueNorm state
            ret, adv = buf.returns.cpu().numpy(), buf.advantages.cpu().numpy()
            vn_state = vn.state.double().cpu().numpy()
    # float64 reference of prepare_loss + clip on the same batch (oracle functions are dtype-generic)
    cfg = H.case_cfg(g)
    hp = po.hyper_from_cfg(cfg)
    d = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    fr = po.flat_rows
    sample = (d(fr(src["policy_obs"][:-1])), d(fr(src["policy_obs"][:-1])), d(fr(src["actions"])),
              d(fr(src["value_preds"][:-1])), d(fr(ret[:-1])), d(fr(src["active_masks"][:-1])),
              d(fr(src["action_log_probs"])), d(adv.reshape(-1, 1)), d(fr(src["action_masks"][:-1])))

    class VN64:  # ValueNorm.normalize with the engine's state (valuenorm.py:79-91) in float64
        def normalize(self, x):
            deb = max(vn_state[2], 1e-5)
            mean, msq = vn_state[0] / deb, vn_state[1] / deb
            return (x - mean) / np.sqrt(max(msq - mean * mean, 1e-2))

        def update(self, x):
            pass

    pth = d(g["theta_p0"]).requires_grad_(True)
    cth = d(g["theta_c0"]).requires_grad_(True)
    pspec, cspec = po.TowerSpec(D, n_act, po.HEAD_CATEGORICAL), po.TowerSpec(D, 1, po.HEAD_VALUE)
    loss_list, *_ = po.prepare_loss(hp, pspec, pth, cspec, cth, VN64(), sample)
    for loss in loss_list:
        loss.backward()
    ref = [po.clip_grad_norm(pth.grad, hp.max_grad_norm)[0], po.clip_grad_norm(cth.grad, hp.max_grad_norm)[0]]
    for k, name in enumerate(("policy", "critic")):
        scale = float(ref[k].abs().max())
        e_split = float((grads["split"][k] - ref[k]).abs().max()) / scale
        e_fp32 = float((grads["fp32"][k] - ref[k]).abs().max()) / scale
        e_pair = float((grads["split"][k] - grads["fp32"][k]).abs().max()) / scale
        print("%s tower: max |g - g64| / max |g64|: split %.3e, fp32 MFMA %.3e; split vs fp32 MFMA %.3e"
              % (name, e_split, e_fp32, e_pair))
        assert e_split < 1e-4 and e_fp32 < 1e-4, (name, e_split, e_fp32)
        assert e_split <= 1.5 * e_fp32 + 2e-7, (name, e_split, e_fp32)
