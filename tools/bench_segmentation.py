"""What a Segmentation observer costs (include/moog_engine.h moog_engine_add_segmentation) against its yardstick, an extra RGB
PILRenderer view of the same size and polygon modifier: both are timed under MOOG_K_VIEWS (HIP events around the derive
launch and the raster launch(es) of that one observer), beside the same primary, 4096 envs.

  colliding_predators_32  64 x 64     colliding_predators_32  128 x 128     chase_avoid_torus  64 x 64, TorusGeometry

The two sides alternate (rgb, seg, rgb, seg, ...) within one process, `--rounds` times each; the table gives every round and
the median.  `--sides rgb` runs the yardstick alone (a build without the observer).  The table replaces the one between the lines `== measurement` and
`== notes` of `--out` (profiles/segmentation.txt); the file's head -- the static comparison of the device code -- and its
notes are kept.

    python tools/bench_segmentation.py [--envs 4096] [--steps 50] [--rounds 3] [--sides rgb,seg] [--case K] [--out FILE]

Per phase: MOOG_RASTER_STOP=k in the environment makes every raster launch return after phase k (2: load, 3: row records,
4: edges and census, 5: row masks; the frames are then garbage, the times are not); MOOG_RASTER_NO_STATIC=1 draws the RGB
view without its cached prefix picture, as a segmentation always is."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.join(REPO, 'moog.github.io_amd'))

CASES = [('colliding_predators_32', (64, 64), False), ('colliding_predators_32', (128, 128), False), ('chase_avoid_torus', (64, 64), True)]
MARK = '== measurement'
NOTES = '== notes'   # (what the file says about the table, and the headline runs: kept)


def config(name, size, torus, side):
    from moog import observers
    from moog_demos import example_configs
    cfg = example_configs.load(name)
    primary = cfg['observers']['image']
    modifier = primary.polygon_modifier if torus else None
    if side == 'rgb':
        extra = observers.PILRenderer(image_size=size, anti_aliasing=1, color_to_rgb='hsv_to_rgb', polygon_modifier=modifier)
    else:
        extra = observers.Segmentation(image_size=size, polygon_modifier=modifier)
    cfg['observers'] = {'image': primary, 'extra': extra}
    return cfg


def timed(env, steps):
    import torch
    from moog import _abi
    for _ in range(5):
        env.step(env.random_action())
    env.set_timing(True)
    for k in range(_abi.MOOG_K_COUNT):
        env.kernel_time(k)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        env.step(env.random_action())
    torch.cuda.synchronize()
    out = {'ms_per_call': (time.perf_counter() - t) * 1e3 / steps}
    for name in ('STEP', 'RASTER', 'VIEWS'):
        ms, _ = env.kernel_time(getattr(_abi, 'MOOG_K_' + name))
        out[name.lower() + '_us'] = 1e3 * ms / steps
    env.set_timing(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--sides', default='rgb,seg')
    ap.add_argument('--case', type=int, default=-1, help='one of the three cases (0, 1, 2) instead of all')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'segmentation.txt'))
    args = ap.parse_args()
    import torch
    from moog import environment
    torch.manual_seed(0)
    sides = args.sides.split(',')
    lines = ['%s tools/bench_segmentation.py on %s: %d envs, %d timed step() calls per round, %d rounds per side, sides alternating'
             % (MARK, torch.cuda.get_device_name(0), args.envs, args.steps, args.rounds),
             'MOOG_K_VIEWS = the derive launch + the raster (+ crop) launch of the one extra observer; us per call',
             '%-24s %-9s %-5s %-28s %8s %9s %10s %9s' % ('workload', 'size', 'side', 'views us by round', 'median', 'step us', 'raster us', 'ms/call')]
    for name, size, torus in (CASES if args.case < 0 else CASES[args.case:args.case + 1]):
        envs = {}
        for side in sides:
            envs[side] = environment.BatchedEnvironment(num_envs=args.envs, seed=1, **config(name, size, torus, side))
            envs[side].check_faults = False
            envs[side].reset()
        runs = {side: [] for side in sides}
        for _ in range(args.rounds):
            for side in sides:
                runs[side].append(timed(envs[side], args.steps))
        for side in sides:
            v = [r['views_us'] for r in runs[side]]
            med = lambda key: statistics.median(r[key] for r in runs[side])
            lines.append('%-24s %-9s %-5s %-28s %8.1f %9.1f %10.1f %9.3f' % (
                name + (' torus' if torus else ''), '%dx%d' % size, side, ' '.join('%.1f' % x for x in v), statistics.median(v),
                med('step_us'), med('raster_us'), med('ms_per_call')))
            envs[side].close()
        print('\n'.join(lines[-len(sides):]), flush=True)
    head = tail = ''
    if os.path.exists(args.out):
        old = open(args.out).read()
        head = old.split(MARK)[0]
        tail = old[old.index(NOTES):] if NOTES in old else ''
    with open(args.out, 'w') as f:
        f.write(head + '\n'.join(lines) + '\n' + tail)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
