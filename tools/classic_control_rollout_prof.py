"""Fused chain rollouts with the default towers: Acrobot-v1 (rollout2_kernel<8, 1, 6, 2>) at 4096
envs x 500 steps next to the synthetic fixed-step env at the same shape (obs 6: rollout2_kernel<8, 1, 0, 0>), and
MountainCar-v0 (rollout2_kernel<8, 1, 7, 1>) at 4096 x 200 next to the synthetic env at obs 2 (rollout2_kernel<8, 1, 0, 0>
as well: the synthetic env's Discrete(3) instance takes the observation width at run time), both with a Discrete(3) head;
MountainCarContinuous-v0 (rollout2_kernel<2, 2, 8, 1>) at 4096 x 200 next to the synthetic env at obs 2 with the same
Box(1) Gaussian head (rollout2_kernel<2, 2, 0, 0>).  `--reps` rollouts each after
one warm-up.  Meant to run under `rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/classic_control_rollout_prof.py --pair acrobot` (one pair per run, so that the two rows of the kernel statistics are
the two envs).  Also prints a host-timed ms
per rollout of each."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAIRS = {"acrobot": ("Acrobot-v1", 6, 500), "mountaincar": ("MountainCar-v0", 2, 200),
         "mountaincar_continuous": ("MountainCarContinuous-v0", 2, 200)}


def rollouts(env_id, D, N, T, reps, box=False, dev="cuda:0"):
    import numpy as np
    import torch

    from openrl_amd import spaces
    from openrl_amd.algorithms.ppo import PPOAlgorithm
    from openrl_amd.buffers import NormalReplayBuffer
    from openrl_amd.configs.config import default_cfg
    from openrl_amd.drivers.onpolicy_driver import OnPolicyDriver
    from openrl_amd.envs.common import make
    from openrl_amd.modules.common import PPONet

    cfg = default_cfg(["--seed", "0", "--episode_length", str(T)])
    act = spaces.Box(-1.0, 1.0, (1,), np.float32) if box else spaces.Discrete(3)
    kw = {} if not env_id.startswith("Synthetic") else dict(obs_dim=D, episode_limit=T, action_space=act)
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
    ap.add_argument("--pair", choices=sorted(PAIRS), default="acrobot")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    env_id, D, T = PAIRS[a.pair]
    box = a.pair == "mountaincar_continuous"
    out = {e: round(rollouts(e, D, a.envs, T, a.reps, box), 4) for e in ("SyntheticFixedStep-v0", env_id)}
    print(json.dumps({"ms_per_rollout_host_timed": out, "obs_dim": D, "envs": a.envs, "T": T, "reps": a.reps}))


if __name__ == "__main__":
    main()
