"""What a recorded rollout costs and buys (BatchedEnvironment.rollout(record=...), include/moog_engine.h
moog_engine_set_table_trajectory).  Two parts, one JSON line per measurement:

  --part a   per (recipe, T), on a config with the default-column float32 SpriteTable over all layers: env-steps per second of
               loop     T step() calls with the table bound (how the states of a roll-out were read before),
               record   one rollout(record='table') call with the same T actions,
               plain    one rollout() call on the same engine, nothing recorded,
             and the HIP-event time of the step kernel (MOOG_K_STEP) per env-step of each: record - plain is the recorder's cost.
  --part b   the paths that record nothing, on the recipes as they are (no table): `step` one step() call per env-step,
             `repeat4` step() at action_repeat=4, `rollout4` / `rollout16` rollout() without record.  --pkg DIR runs it on
             another build of the package (the parent commit's): alternate the two builds in one visit, five runs each, and
             compare the medians with the other build's min - max spread.

Same seeds and pre-drawn random actions in every leg, frames on, cost-ordered launch on (as bench.py runs), at least
--min-steps timed env-steps per leg after the warm-up.

    python tools/bench_rollout_trajectory.py --part a [--recipes pong,chase_avoid_torus,colliding_predators_32] [--envs 4096] [--T 4,16]
    python tools/bench_rollout_trajectory.py --part b [--recipes colliding_predators_32] [--label branch] [--pkg DIR]"""
import argparse
import json
import os
import sys
import time


def timed(env, run, warm, batch, T, n):
    """Runs `run` over the warm-up and then the timed calls: wall time and the step kernel's event time per env-step."""
    import torch
    from moog import _abi
    run(warm)
    env.set_timing(True)
    for kid in range(_abi.MOOG_K_COUNT):
        env.kernel_time(kid)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(batch)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    step_ms, launches = env.kernel_time(_abi.MOOG_K_STEP)
    tables_ms, _ = env.kernel_time(_abi.MOOG_K_TABLES)
    env.set_timing(False)
    steps = len(batch) * T
    return {'wall_s': round(wall, 4), 'env_steps_per_s': round(steps * n / wall, 1),
            'step_kernel_us_per_env_step': round(1e3 * step_ms / steps, 2),
            'tables_us_per_env_step': round(1e3 * tables_ms / steps, 2), 'step_launches': int(launches)}


def make(environment, example_configs, recipe, n, table, **kw):
    from moog import observers
    cfg = example_configs.load(recipe)
    if table:
        cfg['observers'] = dict(cfg['observers'], table=observers.SpriteTable())
    env = environment.BatchedEnvironment(num_envs=n, seed=1, layer_capacity=example_configs.capacity(recipe), **cfg, **kw)
    env.check_faults = False
    env.enable_cost_schedule()
    env.reset()
    return env


def actions(env, T, calls):
    import torch
    torch.manual_seed(T)
    return [torch.stack([env.random_action() for _ in range(T)]) for _ in range(calls)]


def part_a(environment, example_configs, recipe, n, T, min_steps, warmup):
    macro = -(-min_steps // T)
    row = {'part': 'a', 'recipe': recipe, 'num_envs': n, 'T': T}
    for kind in ('loop', 'record', 'plain'):
        env = make(environment, example_configs, recipe, n, True)
        acts = actions(env, T, warmup + macro)

        def run(batch):
            for seq in batch:
                if kind == 'loop':
                    for t in range(T):
                        env.step(seq[t])
                elif kind == 'record':
                    env.rollout(seq, record='table')
                else:
                    env.rollout(seq)
        row[kind] = timed(env, run, acts[:warmup], acts[warmup:], T, n)
        row['step_kernel'] = env.step_kernel()
        row['table_shape'] = list(env.tables['table'].shape[1:])
        env.close()
    row['record_over_loop'] = round(row['record']['env_steps_per_s'] / row['loop']['env_steps_per_s'], 3)
    row['recorder_us_per_env_step'] = round(row['record']['step_kernel_us_per_env_step'] - row['plain']['step_kernel_us_per_env_step'], 2)
    return row


def part_b(environment, example_configs, recipe, n, min_steps, warmup, label):
    row = {'part': 'b', 'label': label, 'recipe': recipe, 'num_envs': n}
    for kind, T, kw in (('step', 1, {}), ('repeat4', 4, {'action_repeat': 4}), ('rollout4', 4, {}), ('rollout16', 16, {})):
        env = make(environment, example_configs, recipe, n, False, **kw)
        macro = -(-min_steps // T)
        acts = actions(env, T, warmup + macro)

        def run(batch):
            for seq in batch:
                if kind.startswith('rollout'):
                    env.rollout(seq)
                else:
                    env.step(seq[0])
        row[kind] = timed(env, run, acts[:warmup], acts[warmup:], T, n)
        row['step_kernel'] = env.step_kernel()
        env.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='a', choices=('a', 'b'))
    ap.add_argument('--recipes', default=None)
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--T', default='4,16')
    ap.add_argument('--min-steps', type=int, default=240, help='timed env-steps per leg (at least 240)')
    ap.add_argument('--warmup', type=int, default=10, help='calls before the timed loop')
    ap.add_argument('--label', default='branch', help='(part b) names the build in the output')
    ap.add_argument('--pkg', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'moog.github.io_amd'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    from moog import environment
    from moog_demos import example_configs
    min_steps = max(240, args.min_steps)
    if args.part == 'a':
        for recipe in (args.recipes or 'pong,chase_avoid_torus,colliding_predators_32').split(','):
            for T in (int(x) for x in args.T.split(',')):
                print(json.dumps(part_a(environment, example_configs, recipe, args.envs, T, min_steps, args.warmup)), flush=True)
    else:
        for recipe in (args.recipes or 'colliding_predators_32').split(','):
            print(json.dumps(part_b(environment, example_configs, recipe, args.envs, min_steps, args.warmup, args.label)), flush=True)


if __name__ == '__main__':
    main()
