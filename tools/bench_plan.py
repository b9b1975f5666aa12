"""What candidate rollouts buy (BatchedEnvironment.rollout_candidates, include/moog_engine.h moog_engine_plan_sequences): for a
recipe, a batch size, K candidates and T steps, candidate-env-steps per second (K x T x N per plan) of

    plan      one rollout_candidates() call,
    rollouts  (a) K x (raw copy-back of both state tensors + rollout()) on the same engine: today's way at its cheapest, and
    big       (b) an engine of K x N envs filled by a replicating copy of the N records, then one rollout(),

all on engines whose only observer is a RawState (no frames, tables or sensors: nothing a planner discards is drawn), same
seed, the same random actions drawn ahead of the timed loop, --runs runs of --plans plans each after a warm-up.  Beside the
wall time: the HIP-event time of the step kernel (MOOG_K_STEP) per candidate-env-step.  One JSON line per (recipe, K, T)
with the median and the min - max of the runs.

    python tools/bench_plan.py [--recipes pong,chase_avoid_torus,colliding_predators_32] [--envs 4096] [--K 4,16,64] [--T 4,16]
                               [--legs plan,rollouts,big] [--runs 5] [--plans 8] [--pkg DIR]"""
import argparse
import json
import os
import statistics
import sys
import time


def make(environment, example_configs, observers, recipe, n):
    cfg = example_configs.load(recipe)
    cfg['observers'] = {'state': observers.RawState()}
    env = environment.BatchedEnvironment(num_envs=n, seed=1, layer_capacity=example_configs.capacity(recipe), **cfg)
    env.check_faults = False
    env.enable_cost_schedule()
    env.reset()
    return env


def leg(mods, recipe, n, K, T, kind, runs, plans, warmup):
    import torch
    from moog import _abi
    environment, example_configs, observers = mods
    env = make(environment, example_configs, observers, recipe, n)
    for _ in range(4):   # (a few real steps: the states differ from a reset)
        env.step(env.random_action())
    big = make(environment, example_configs, observers, recipe, n * K) if kind == 'big' else None
    torch.manual_seed(K * 1000 + T)
    acts = [torch.stack([torch.stack([env.random_action() for _ in range(T)]) for _ in range(K)]) for _ in range(warmup + plans)]
    if big is not None:   # [K, T, N, ...] -> [T, K x N, ...]: env k N + e of the big engine runs candidate k of env e
        acts = [a.transpose(0, 1).reshape((T, K * n) + tuple(a.shape[3:])).contiguous() for a in acts]

    def plan(a):
        if kind == 'plan':
            env.rollout_candidates(a)
        elif kind == 'rollouts':
            f, q = env.state_f64.clone(), env.state_i32.clone()
            for k in range(K):
                env.rollout(a[k])
                env.state_f64.copy_(f)
                env.state_i32.copy_(q)
        else:
            big.state_f64.view(K, n, -1).copy_(env.state_f64.unsqueeze(0))
            big.state_i32.view(K, n, -1).copy_(env.state_i32.unsqueeze(0))
            big.rollout(a)

    timed = big if big is not None else env
    for a in acts[:warmup]:
        plan(a)
    walls, kernels = [], []
    for _ in range(runs):
        timed.set_timing(True)
        timed.kernel_time(_abi.MOOG_K_STEP)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for a in acts[warmup:]:
            plan(a)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        kernels.append(timed.kernel_time(_abi.MOOG_K_STEP)[0])
        timed.set_timing(False)
    work = plans * K * T * n
    rate = sorted(work / w for w in walls)
    out = {'cand_env_steps_per_s': round(statistics.median(rate), 1), 'min': round(rate[0], 1), 'max': round(rate[-1], 1),
           'step_kernel_ns_per_cand_env_step': round(1e6 * statistics.median(kernels) / work, 3),
           'kernel': env.plan_kernel() if kind == 'plan' else timed.step_kernel()}
    env.close()
    if big is not None:
        big.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--recipes', default='pong,chase_avoid_torus,colliding_predators_32')
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--K', default='4,16,64')
    ap.add_argument('--T', default='4,16')
    ap.add_argument('--legs', default='plan,rollouts,big')
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--plans', type=int, default=8, help='timed plans per run')
    ap.add_argument('--warmup', type=int, default=2, help='plans before the timed runs')
    ap.add_argument('--pkg', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'moog.github.io_amd'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    from moog import environment, observers
    from moog_demos import example_configs
    mods = (environment, example_configs, observers)
    for recipe in args.recipes.split(','):
        for K in (int(x) for x in args.K.split(',')):
            for T in (int(x) for x in args.T.split(',')):
                row = {'recipe': recipe, 'num_envs': args.envs, 'K': K, 'T': T}
                for name in args.legs.split(','):
                    row[name] = leg(mods, recipe, args.envs, K, T, name, args.runs, args.plans, args.warmup)
                for base in ('rollouts', 'big'):
                    if 'plan' in row and base in row:
                        row['plan_over_' + base] = round(row['plan']['cand_env_steps_per_s'] / row[base]['cand_env_steps_per_s'], 3)
                print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
