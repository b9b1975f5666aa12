"""What a SpriteTable observer costs (include/moog_engine.h moog_engine_add_table) and what it replaces: pong,
chase_avoid_torus (no renderer: the shape of bench.py --phase step) and colliding_predators_32 at 4096 envs, stepped without
and with the default table -- ms per call and the HIP-event time of MOOG_K_TABLES per call -- and, on the same visit, the same
tensor assembled by torch from `env.field()` views as a user writes it today (stack / cat, .float(), masked by alive).
Also the bytes the table launch moves and the GB/s that makes of its event time.

    python tools/bench_sprite_table.py [--envs 4096] [--steps 200] [--out profiles/sprite_table.txt]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'moog.github.io_amd'))

WORKLOADS = ('pong', 'chase_avoid_torus', 'colliding_predators_32')


def config(name, table):
    from moog import observers
    from moog_demos import example_configs
    cfg = example_configs.load(name)
    obs = {} if name == 'chase_avoid_torus' else dict(cfg['observers'])
    if name == 'chase_avoid_torus':
        obs['state'] = observers.RawState()
    if table:
        obs['table'] = observers.SpriteTable(dtype=table)
    cfg['observers'] = obs
    return cfg


def torch_table(env, torch):
    """The default table from field() views, as a caller assembles it without the observer."""
    pos, vel, col = env.field('position'), env.field('velocity'), env.field('color')
    alive = env.field('alive')
    cols = [alive.double(), pos[:, :, 0], pos[:, :, 1], vel[:, :, 0], vel[:, :, 1], env.field('angle'), env.field('angle_vel'),
            col[:, :, 0], col[:, :, 1], col[:, :, 2], env.field('opacity').double(), env.field('mass')]
    return torch.stack(cols, dim=2).float() * alive.unsqueeze(2)


def wall(torch, call, steps):
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from moog import _abi, environment
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say('%d envs, %d timed calls each; %s' % (args.envs, args.steps, torch.cuda.get_device_name(0)))
    say('%-24s %-8s %9s %10s %11s %9s %8s' % ('workload', 'table', 'ms/call', 'tables us', 'torch us', 'MB moved', 'GB/s'))
    for name in WORKLOADS:
        for table in (None, 'float32', 'float16'):
            torch.manual_seed(0)
            env = environment.BatchedEnvironment(num_envs=args.envs, seed=1, **config(name, table))
            env.check_faults = False
            env.reset()
            acts = [env.random_action() for _ in range(8)]
            k = [0]

            def step():
                k[0] += 1
                env.step(acts[k[0] % 8])
            ms = wall(torch, step, args.steps)
            if table is None:
                # the same tensor from field() views, on this state: torch launches only (no step)
                tus = 1e3 * wall(torch, lambda: torch_table(env, torch), args.steps)
                say('%-24s %-8s %9.4f %10s %11.1f' % (name, '-', ms, '', tus))
                env.close()
                continue
            env.set_timing(True, kernels=[_abi.MOOG_K_TABLES])
            env.kernel_time(_abi.MOOG_K_TABLES)
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            kms, n = env.kernel_time(_abi.MOOG_K_TABLES)
            env.set_timing(False)
            us = 1e3 * kms / max(1, n)
            t = env.tables['table']
            rows, cols = t.shape[1], t.shape[2]
            # read: the flag word of every row and the value of every element (8 bytes, 4 for opacity; `alive` reads none);
            # written: the table
            moved = args.envs * (rows * 4 + rows * (10 * 8 + 4) + t[0].numel() * t.element_size())
            note = ''
            if table == 'float32':
                same = torch.equal(torch.nan_to_num(torch_table(env, torch)), torch.nan_to_num(t))
                note = '   equals the torch composition: %s' % same
            say('%-24s %-8s %9.4f %10.1f %11s %9.2f %8.1f   [%d x %d]%s' % (name, table, ms, us, '', moved / 1e6, moved / 1e3 / us, rows, cols, note))
            env.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
