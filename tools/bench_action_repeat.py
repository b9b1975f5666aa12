"""What action repeat buys (BatchedEnvironment(action_repeat=k), include/moog_engine.h moog_engine_set_action_repeat): for a
recipe, a batch size and a list of k, env-steps per second of

    loop    k step() calls per held action on an engine with action_repeat = 1 (what a training loop did before), and
    repeat  one step() call per held action on an engine with action_repeat = k,

same build, same seeds, the same random actions (drawn ahead of the timed loop, one per k env-steps in both legs), frames on,
cost-ordered launch on (as bench.py runs), at least --min-steps timed env-steps per leg after the warm-up.  Beside the wall
time: the HIP-event time of the step kernel (MOOG_K_STEP) and of the primary's frames (MOOG_K_RASTER) per env-step, and the
mean number of env-steps an env took per call of the warm-up (below k where episodes ended inside a call, or a call reset the env).
One JSON line per (recipe, k).

    python tools/bench_action_repeat.py [--recipes pong,chase_avoid_torus,colliding_predators_32] [--envs 4096] [--k 2,4,8]
                                        [--legs loop,repeat] [--pkg DIR]

--legs loop runs on a tree that has no action repeat too (--pkg: that tree's package directory), which is how the loop of an
older build is measured beside this build's repeat."""
import argparse
import json
import os
import sys
import time


def leg(environment, example_configs, recipe, n, k, repeat, min_steps, warmup):
    import torch
    from moog import _abi
    kw = {'action_repeat': k} if repeat else {}
    env = environment.BatchedEnvironment(num_envs=n, seed=1, layer_capacity=example_configs.capacity(recipe),
                                         **example_configs.load(recipe), **kw)
    env.check_faults = False
    env.enable_cost_schedule()
    env.reset()
    macro = -(-min_steps // k)
    torch.manual_seed(k)
    acts = [env.random_action() for _ in range(warmup + macro)]
    calls = 1 if repeat else k

    def run(batch, count=False):
        taken = 0
        for a in batch:
            for _ in range(calls):
                env.step(a)
                if count:
                    taken = taken + env.repeat_count.sum()
        return taken

    taken = run(acts[:warmup], count=repeat)   # (counted in the warm-up only: the timed loop holds nothing but step calls)
    env.set_timing(True)
    for kid in range(_abi.MOOG_K_COUNT):
        env.kernel_time(kid)
    torch.cuda.synchronize()
    t = time.perf_counter()
    run(acts[warmup:])
    torch.cuda.synchronize()
    wall = time.perf_counter() - t
    step_ms, launches = env.kernel_time(_abi.MOOG_K_STEP)
    raster_ms, _ = env.kernel_time(_abi.MOOG_K_RASTER)
    env.set_timing(False)
    # env-steps the batch was asked for (the loop's calls that reset an env count as one, as a training loop counts them)
    asked = macro * k * n
    out = {'calls': macro * calls, 'wall_s': round(wall, 4), 'env_steps_per_s': round(asked / wall, 1),
           'step_kernel_us_per_env_step': round(1e3 * step_ms / (macro * k), 2),
           'raster_us_per_env_step': round(1e3 * raster_ms / (macro * k), 2),
           'step_kernel_us_per_launch': round(1e3 * step_ms / max(1, launches), 2), 'step_kernel': env.step_kernel()}
    if repeat:
        out['env_steps_taken_per_call'] = round(float(taken) / (warmup * n), 3)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--recipes', default='pong,chase_avoid_torus,colliding_predators_32')
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--k', default='2,4,8')
    ap.add_argument('--legs', default='loop,repeat')
    ap.add_argument('--min-steps', type=int, default=240, help='timed env-steps per leg (at least 200)')
    ap.add_argument('--warmup', type=int, default=10, help='held actions before the timed loop')
    ap.add_argument('--pkg', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'moog.github.io_amd'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    from moog import environment
    from moog_demos import example_configs
    legs = args.legs.split(',')
    for recipe in args.recipes.split(','):
        for k in (int(x) for x in args.k.split(',')):
            row = {'recipe': recipe, 'num_envs': args.envs, 'k': k}
            for name in legs:
                row[name] = leg(environment, example_configs, recipe, args.envs, k, name == 'repeat', max(200, args.min_steps), args.warmup)
            if 'loop' in row and 'repeat' in row:
                row['repeat_over_loop'] = round(row['repeat']['env_steps_per_s'] / row['loop']['env_steps_per_s'], 3)
            print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
