"""What extra views cost (include/moog_engine.h moog_engine_add_view): colliding_predators_32 at 4096 envs, stepped with
frames four ways -- one view; plus a 64 x 64 first-person view; plus a 128 x 128 view; plus a 256 x 256 view (the span
kernel) -- ms per call and the HIP-event times of MOOG_K_STEP / MOOG_K_RASTER (the primary's frames) / MOOG_K_VIEWS (the
extra views' derive launch and raster launches).  Then each extra renderer ALONE in a one-view engine, drawn by
moog_engine_render (its derive + raster launches under MOOG_K_RASTER): the yardstick for what the same view costs as an
extra view.

    python tools/bench_views.py [--envs 4096] [--steps 50]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'moog.github.io_amd'))

EXTRA = [('fp64', dict(image_size=(64, 64), anti_aliasing=1, color_to_rgb='hsv_to_rgb', first_person=True)),
         ('v128', dict(image_size=(128, 128), anti_aliasing=1, color_to_rgb='hsv_to_rgb')),
         ('v256', dict(image_size=(256, 256), anti_aliasing=1, color_to_rgb='hsv_to_rgb'))]


def renderer(spec):
    from moog import observers
    from moog.observers import polygon_modifiers
    spec = dict(spec)
    if spec.pop('first_person', False):
        spec['polygon_modifier'] = polygon_modifiers.FirstPersonAgent(agent_layer='agent')
    return observers.PILRenderer(**spec)


def config(extra):
    from moog_demos import example_configs
    cfg = example_configs.load('colliding_predators_32')
    obs = {'image': cfg['observers']['image']}
    for key, spec in extra:
        obs[key] = renderer(spec)
    cfg['observers'] = obs
    return cfg


def timed(env, call, steps):
    import torch
    from moog import _abi
    for _ in range(5):
        call()
    env.set_timing(True)
    for k in range(_abi.MOOG_K_COUNT):
        env.kernel_time(k)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        call()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t) * 1e3 / steps
    out = {'ms_per_call': wall}
    for name in ('STEP', 'RASTER', 'VIEWS'):
        ms, n = env.kernel_time(getattr(_abi, 'MOOG_K_' + name))
        out[name.lower() + '_us'] = 1e3 * ms / steps
    env.set_timing(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=50)
    args = ap.parse_args()
    import torch
    from moog import environment
    torch.manual_seed(0)
    print('colliding_predators_32, %d envs, %d timed calls each; per call: wall ms, HIP-event us of the kernels' % (args.envs, args.steps))
    print('%-28s %9s %9s %10s %9s   %s' % ('step with frames', 'ms/call', 'step us', 'raster us', 'views us', 'paths'))
    for k in range(len(EXTRA) + 1):
        env = environment.BatchedEnvironment(num_envs=args.envs, seed=1, **config(EXTRA[:k]))
        env.check_faults = False
        env.reset()
        r = timed(env, lambda: env.step(env.random_action()), args.steps)
        paths = ' '.join('%s=%s' % (key, env.raster_path(key)) for key in ['image'] + [e[0] for e in EXTRA[:k]])
        print('%-28s %9.3f %9.1f %10.1f %9.1f   %s' % ('image' + ''.join(' + ' + e[0] for e in EXTRA[:k]), r['ms_per_call'],
                                                      r['step_us'], r['raster_us'], r['views_us'], paths), flush=True)
        if k == len(EXTRA):   # the render call of the 4-view engine: the primary's records join the extra views' derive launch
            rr = timed(env, env.observation, args.steps)
            print('%-28s %9.3f %9s %10.1f %9.1f' % ('  render (4 views)', rr['ms_per_call'], '', rr['raster_us'], rr['views_us']))
        env.close()
    print('each extra view by itself beside the primary (MOOG_K_VIEWS: that one view\'s derive + raster launches):')
    for k in range(len(EXTRA)):
        env = environment.BatchedEnvironment(num_envs=args.envs, seed=1, **config(EXTRA[k:k + 1]))
        env.check_faults = False
        env.reset()
        r = timed(env, lambda: env.step(env.random_action()), args.steps)
        print('%-28s %9.3f %9.1f %10.1f %9.1f   %s' % ('image + ' + EXTRA[k][0], r['ms_per_call'], r['step_us'], r['raster_us'],
                                                      r['views_us'], env.raster_path(EXTRA[k][0])), flush=True)
        env.close()
    print('one-view engines, moog_engine_render (derive + raster of that renderer alone, MOOG_K_RASTER); "repeated": render calls '
          'one after another on the same state, "after step": every render call follows a step without frames (new state, as '
          'in a step with frames)')
    for key, spec in EXTRA:
        cfg = config([])
        cfg['observers'] = {key: renderer(spec)}
        env = environment.BatchedEnvironment(num_envs=args.envs, seed=1, **cfg)
        env.check_faults = False
        env.reset()
        for _ in range(5):
            env.step(env.random_action())
        r = timed(env, env.observation, args.steps)
        out = env._out   # (a step that draws no frames: the engine's step call without the image)
        noimg = type(out)()
        noimg.reward, noimg.discount, noimg.step_type = out.reward, out.discount, out.step_type
        env._out = noimg

        def step_then_render():
            env.step(env.random_action())
            env.observation()
        r2 = timed(env, step_then_render, args.steps)
        env._out = out
        print('%-28s %9.3f %9s %10.1f   repeated   %s' % ('  ' + key + ' alone', r['ms_per_call'], '', r['raster_us'], env.raster_path()))
        print('%-28s %9.3f %9.1f %10.1f   after step' % ('  ' + key + ' alone', r2['ms_per_call'], r2['step_us'], r2['raster_us']), flush=True)
        env.close()


if __name__ == '__main__':
    main()
