"""What an open-loop rollout buys (BatchedEnvironment.rollout, include/moog_engine.h moog_engine_step_sequence): for a recipe, a
batch size and a list of T, env-steps per second of

    loop     T step() calls with T different actions (what a planner's roll-out did before),
    rollout  one rollout() call with the same T actions, and
    repeat   one step() call on an engine with action_repeat = T: the same kernel with ONE action, the yardstick for what the
             per-step action reads and reward stores cost,

same build, same seeds, the same random actions (drawn ahead of the timed loop: [T, N, ...] per call; the repeat leg holds the
first of each T), frames on, cost-ordered launch on (as bench.py runs), at least --min-steps timed env-steps per leg after the
warm-up.  Beside the wall time: the HIP-event time of the step kernel (MOOG_K_STEP) and of the primary's frames
(MOOG_K_RASTER) per env-step, and the mean number of env-steps an env took per call of the warm-up.  One JSON line per
(recipe, T).

    python tools/bench_rollout.py [--recipes pong,chase_avoid_torus,colliding_predators_32] [--envs 4096] [--T 4,16]
                                  [--legs loop,rollout,repeat] [--pkg DIR]"""
import argparse
import json
import os
import sys
import time


def leg(environment, example_configs, recipe, n, T, kind, min_steps, warmup):
    import torch
    from moog import _abi
    kw = {'action_repeat': T} if kind == 'repeat' else {}
    env = environment.BatchedEnvironment(num_envs=n, seed=1, layer_capacity=example_configs.capacity(recipe),
                                         **example_configs.load(recipe), **kw)
    env.check_faults = False
    env.enable_cost_schedule()
    env.reset()
    macro = -(-min_steps // T)
    torch.manual_seed(T)
    acts = [torch.stack([env.random_action() for _ in range(T)]) for _ in range(warmup + macro)]

    def run(batch, count=False):
        taken = 0
        for seq in batch:
            if kind == 'loop':
                for t in range(T):
                    env.step(seq[t])
            elif kind == 'rollout':
                env.rollout(seq)
            else:
                env.step(seq[0])
            if count and kind != 'loop':
                taken = taken + env.repeat_count.sum()
        return taken

    taken = run(acts[:warmup], count=True)   # (counted in the warm-up only: the timed loop holds nothing but the calls)
    env.set_timing(True)
    for kid in range(_abi.MOOG_K_COUNT):
        env.kernel_time(kid)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(acts[warmup:])
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    step_ms, launches = env.kernel_time(_abi.MOOG_K_STEP)
    raster_ms, _ = env.kernel_time(_abi.MOOG_K_RASTER)
    env.set_timing(False)
    # env-steps the batch was asked for (the loop's calls that reset an env count as one, as a training loop counts them)
    asked = macro * T * n
    calls = macro * (T if kind == 'loop' else 1)
    out = {'calls': calls, 'wall_s': round(wall, 4), 'env_steps_per_s': round(asked / wall, 1),
           'step_kernel_us_per_env_step': round(1e3 * step_ms / (macro * T), 2),
           'raster_us_per_env_step': round(1e3 * raster_ms / (macro * T), 2),
           'step_kernel_us_per_launch': round(1e3 * step_ms / max(1, launches), 2), 'step_kernel': env.step_kernel()}
    if kind != 'loop':
        out['env_steps_taken_per_call'] = round(float(taken) / (warmup * n), 3)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--recipes', default='pong,chase_avoid_torus,colliding_predators_32')
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--T', default='4,16')
    ap.add_argument('--legs', default='loop,rollout,repeat')
    ap.add_argument('--min-steps', type=int, default=240, help='timed env-steps per leg (at least 240)')
    ap.add_argument('--warmup', type=int, default=10, help='calls (of T env-steps) before the timed loop')
    ap.add_argument('--pkg', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'moog.github.io_amd'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    from moog import environment
    from moog_demos import example_configs
    legs = args.legs.split(',')
    for recipe in args.recipes.split(','):
        for T in (int(x) for x in args.T.split(',')):
            row = {'recipe': recipe, 'num_envs': args.envs, 'T': T}
            for name in legs:
                row[name] = leg(environment, example_configs, recipe, args.envs, T, name, max(240, args.min_steps), args.warmup)
            if 'loop' in row and 'rollout' in row:
                row['rollout_over_loop'] = round(row['rollout']['env_steps_per_s'] / row['loop']['env_steps_per_s'], 3)
            if 'repeat' in row and 'rollout' in row:
                row['rollout_over_repeat'] = round(row['rollout']['env_steps_per_s'] / row['repeat']['env_steps_per_s'], 3)
            print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
