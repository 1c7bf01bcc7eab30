"""Fused chain rollouts at 4096 envs x 200 steps, obs 3, Box(1), default towers: Pendulum-v1 (rollout2_kernel<2, 2, 5, 1>)
and the synthetic fixed-step env at the same shape (rollout2_kernel<2, 2, 0, 0>), `--reps` rollouts each after one warm-up.
Meant to run under `rocprofv3 --kernel-trace --stats -- python tools/pendulum_rollout_prof.py`: the two kernel instances
appear as separate rows of the kernel statistics.  Also prints a host-timed ms per rollout of each."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rollouts(env_id, N, T, reps, dev="cuda:0"):
    import torch

    from openrl_amd import spaces
    from openrl_amd.algorithms.ppo import PPOAlgorithm
    from openrl_amd.buffers import NormalReplayBuffer
    from openrl_amd.configs.config import default_cfg
    from openrl_amd.drivers.onpolicy_driver import OnPolicyDriver
    from openrl_amd.envs.common import make
    from openrl_amd.modules.common import PPONet

    cfg = default_cfg(["--seed", "0", "--episode_length", str(T)])
    kw = {} if env_id == "Pendulum-v1" else dict(obs_dim=3, episode_limit=200, action_space=spaces.Box(-2.0, 2.0, (1,)))
    env = make(env_id, env_num=N, device=dev, seed=0, **kw)
    net = PPONet(env, cfg=cfg, device=dev, n_rollout_threads=N)
    cfg.num_env_steps = N * T * (reps + 1)

    class _Agent:
        num_time_steps = 0

    trainer = PPOAlgorithm(cfg, net.module, agent_num=1, device=dev)
    buf = NormalReplayBuffer(cfg, 1, env.observation_space, env.action_space, device=dev)
    drv = OnPolicyDriver({"cfg": cfg, "num_agents": 1, "run_dir": None, "envs": env, "device": dev}, trainer, buf, _Agent())
    assert drv.fused
    drv.reset_and_buffer_init()
    drv.actor_rollout()
    buf.data.after_update()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        drv.actor_rollout()
        buf.data.after_update()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    out = {env_id: round(rollouts(env_id, a.envs, a.T, a.reps), 4) for env_id in ("SyntheticFixedStep-v0", "Pendulum-v1")}
    print(json.dumps({"ms_per_rollout_host_timed": out, "envs": a.envs, "T": a.T, "reps": a.reps}))


if __name__ == "__main__":
    main()
