"""End-to-end PPO iterations on the device classic-control envs, default recipe (ppo_epoch 10, num_mini_batch 1, hidden
64), fused chain rollout: Acrobot-v1 at 4096 envs x 500 and MountainCar-v0 at 4096 envs x 200 with a Discrete(3) head,
MountainCarContinuous-v0 at 4096 envs x 200 with a Box(1) Gaussian head.
Stand-alone (bench.py does not run it); one JSON line per env:

    python benchmarks/classic_control.py [--steps 3 --warmup 2]

Measured with benchmarks/other_configs.py's ``measure`` (ms per iteration, env-steps/s, the update's dominant kernel)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = [
    dict(name="Acrobot-v1, PPO, 4096 envs x 500, obs 6, Discrete(3), device env, fused rollout", env="Acrobot-v1",
         envs=4096, T=500, agents=1, env_kw={}, argv=[]),
    dict(name="MountainCar-v0, PPO, 4096 envs x 200, obs 2, Discrete(3), device env, fused rollout", env="MountainCar-v0",
         envs=4096, T=200, agents=1, env_kw={}, argv=[]),
    dict(name="MountainCarContinuous-v0, PPO, 4096 envs x 200, obs 2, Box(1), device env, fused rollout",
         env="MountainCarContinuous-v0", envs=4096, T=200, agents=1, env_kw={}, argv=[]),
]


def main():
    from benchmarks.other_configs import measure

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    for c in CONFIGS:
        print(json.dumps(measure(c, steps=a.steps, warmup=a.warmup)), flush=True)


if __name__ == "__main__":
    main()
