"""Extra views on the MI355X: every PILRenderer of a config drawn by one engine (include/moog_engine.h
moog_engine_add_view) -- against one-view engines, the oracle and the reference's multi-view recordings
(tests/golden/views_zoo_l*.npz); sub-batches, facades, configs without a renderer."""
import numpy as np
import pytest

import helpers
from helpers import OracleEnv, fixture, records_from_fixture
from moog import _compiler, observers
from moog.observers import polygon_modifiers
from moog_demos.example_configs import functional_maze, views_zoo

pytestmark = pytest.mark.gpu


def _env(cfg, n, seed=0, sub_batches=None, **kw):
    from moog import environment
    if sub_batches:
        return environment.SubBatchedEnvironment(num_envs=n, sub_batches=sub_batches, seed=seed, **cfg, **kw)
    return environment.BatchedEnvironment(num_envs=n, seed=seed, **cfg, **kw)


def _only(cfg, key):
    out = dict(cfg)
    out['observers'] = {key: cfg['observers'][key]}
    return out


def _maze_views():
    cfg = functional_maze.get_config(None)   # border walls: a static prefix on both views
    cfg['observers'] = {'image': cfg['observers']['image'],
                        'small': observers.PILRenderer(image_size=(40, 40), anti_aliasing=1)}
    return cfg


def _aa_torus_views():
    # an anti-aliased extra view on the mask path (a 128 x 128 canvas: its records are derived ahead, one chunk covers every
    # env) and a torus extra view (nine copies per sprite: the derive launch's LDS is sized by it)
    cfg = views_zoo.get_config(0)
    cfg['observers'] = {'image': cfg['observers']['image'],
                        'aa': observers.PILRenderer(image_size=(64, 64), anti_aliasing=2, color_to_rgb='hsv_to_rgb'),
                        'torus': observers.PILRenderer(image_size=(64, 64), color_to_rgb='hsv_to_rgb',
                                                       polygon_modifier=polygon_modifiers.TorusGeometry(['predators', 'agent']))}
    return cfg


def _aa_primary_views():
    # an anti-aliased primary on the mask path: its records join the extra view's derive launch on reset and render calls
    cfg = views_zoo.get_config(0)
    cfg['observers'] = {'image': observers.PILRenderer(image_size=(64, 64), anti_aliasing=2, color_to_rgb='hsv_to_rgb'),
                        'small': observers.PILRenderer(image_size=(32, 32), color_to_rgb='hsv_to_rgb')}
    return cfg


def _grey(c):
    return (int(255 * c[0]) % 256, 90, 200)


def _callable_views():
    # the same color_to_rgb callable on both renderers: the views share the host-side colour array
    cfg = views_zoo.get_config(0)
    cfg['observers'] = {'image': observers.PILRenderer(image_size=(64, 64), color_to_rgb=_grey),
                        'big': observers.PILRenderer(image_size=(96, 96), color_to_rgb=_grey)}
    return cfg


CONFIGS = {'l0': lambda: views_zoo.get_config(0), 'l1': lambda: views_zoo.get_config(1),
           'l2': lambda: views_zoo.get_config(2), 'maze': _maze_views, 'aa_torus': _aa_torus_views,
           'aa_primary': _aa_primary_views, 'callable': _callable_views}


def _actions(n, calls, seed=5):
    import torch
    g = torch.Generator().manual_seed(seed)
    return [torch.rand((n, 2), generator=g, dtype=torch.float64) * 2 - 1 for _ in range(calls)]


@pytest.mark.parametrize('which', sorted(CONFIGS))
def test_views_equal_one_view_engines(which):
    """Each view's frames equal, bit for bit, those of a one-view engine with that renderer alone: same seed, same actions,
    256 envs, across episode resets."""
    import torch
    cfg = CONFIGS[which]()
    keys = [k for k, o in cfg['observers'].items() if isinstance(o, observers.PILRenderer)]
    n, calls = 256, 220   # (colliding_predators' episodes time out after 200 steps)
    acts = _actions(n, calls)
    multi = _env(cfg, n)
    singles = {k: _env(_only(cfg, k), n) for k in keys}
    ts = multi.reset()
    outs = {k: e.reset() for k, e in singles.items()}
    assert list(ts.observation) == list(cfg['observers'])
    resets = 0
    for t in range(calls + 1):
        for k in keys:
            assert torch.equal(ts.observation[k], outs[k].observation[k]), (which, k, t)
            assert torch.equal(ts.step_type, outs[k].step_type), (which, k, t)
        if t == calls:
            break
        ts = multi.step(acts[t])
        outs = {k: e.step(acts[t]) for k, e in singles.items()}
        resets += int((ts.step_type == 0).sum().item())
    assert resets > 0, 'no episode ended: the run does not cross a reset'
    # a render call (records derived from the stored state) draws every view again, identically
    obs = multi.observation()
    for k in keys:
        assert torch.equal(obs[k], singles[k].observation()[k]), (which, k)
    for e in [multi] + list(singles.values()):
        e.close()


def test_raster_paths_per_view():
    env = _env(views_zoo.get_config(2), 8)
    assert env.raster_path() == 'mask' and env.raster_path('image') == 'mask'
    assert env.raster_path('big') == 'spans'
    env0 = _env(views_zoo.get_config(0), 8)
    # (an anti-aliased 96 x 96 view draws a 192 x 192 canvas: beyond the mask rasteriser's 128 x 128)
    assert [env0.raster_path(k) for k in ('image', 'ego', 'video')] == ['mask', 'mask', 'spans']
    with pytest.raises(KeyError):
        env0.raster_path('state')
    env.close()
    env0.close()


VIEW_KEYS = {0: ('image', 'ego', 'video'), 1: ('image', 'plain'), 2: ('image', 'big')}


@pytest.mark.parametrize('level', [0, 1, 2])
def test_views_teacher_forced_vs_reference(level):
    """All recorded calls at once (env i starts from the reference state of call i): every view's frame of call i + 1 equals
    the reference's."""
    import test_gpu_parity as tgp
    fx = fixture('views_zoo_l%d' % level)
    cfg = views_zoo.get_config(level)
    c = _compiler.compile_config(**cfg)
    T = len(fx['step_type'])
    ts = list(range(1, T))
    env = _env(cfg, len(ts))
    L = c.layout
    f64 = np.zeros((len(ts), L.f64_per_env))
    i32 = np.zeros((len(ts), L.i32_per_env), np.int32)
    for i, t in enumerate(ts):
        records_from_fixture(fx, t - 1, c, f64, i32, env=i)
    tgp.upload(env, f64, i32)
    env.check_faults = False
    out = env.step(np.stack([helpers.action_of(fx, t) for t in ts]), injected_uniforms=tgp.padded_uniforms(fx, ts))
    for key in VIEW_KEYS[level]:
        img = out.observation[key].cpu().numpy()
        for i, t in enumerate(ts):
            assert int(out.step_type[i]) == int(fx['step_type'][t]), t
            assert np.array_equal(img[i], fx['image_' + key][t]), '%s: frame %d differs' % (key, t)
    env.close()


def _oracle_frames(cfg, key, f64, i32):
    o = OracleEnv(_compiler.compile_config(**_only(cfg, key)), n_envs=f64.shape[0])
    o.f64[:] = f64
    o.i32[:] = i32
    return o.render().copy()


def test_fresh_frames_after_state_changes():
    """load_state, restore, an edit of the state tensors and reset(env_mask): observation() redraws every view, and each
    matches the oracle."""
    import torch
    cfg = views_zoo.get_config(0)
    keys = ('image', 'ego', 'video')
    n = 64
    env = _env(cfg, n, seed=3)
    env.reset()
    for a in _actions(n, 12):
        env.step(a)

    def check(tag):
        obs = env.observation()
        torch.cuda.synchronize()
        f, q = env.state_f64.cpu().numpy(), env.state_i32.cpu().numpy()
        for k in keys:
            assert np.array_equal(obs[k].cpu().numpy(), _oracle_frames(cfg, k, f, q)), (tag, k)
    check('stepped')
    snap = env.snapshot()
    for a in _actions(n, 5, seed=9):
        env.step(a)
    env.restore(snap)
    check('restore')
    L = env.layout
    env.state_f64[:, L.o_pos:L.o_pos + 2 * L.S] += 0.013   # an edit of the state tensors
    check('edit')
    mask = torch.zeros(n, dtype=torch.uint8)
    mask[::3] = 1
    env.reset(env_mask=mask)
    check('reset(env_mask)')
    env.close()


def test_sub_batches_match_batched():
    import torch
    cfg = views_zoo.get_config(0)
    n = 256
    acts = _actions(n, 30)
    one = _env(cfg, n, seed=1)
    two = _env(cfg, n, seed=1, sub_batches=2)
    a, b = one.reset(), two.reset()
    for t in range(31):
        assert list(b.observation) == ['image', 'ego', 'video', 'state']
        for k in ('image', 'ego', 'video'):
            assert torch.equal(a.observation[k], b.observation[k]), (k, t)
        if t < 30:
            a, b = one.step(acts[t]), two.step(acts[t])
    one.close()
    two.close()


def test_environment_and_gym_facades():
    from moog import environment
    from moog.env_wrappers import gym_wrapper
    cfg = views_zoo.get_config(0)
    env = environment.Environment(**cfg)
    ts = env.reset()
    assert list(ts.observation) == ['image', 'ego', 'video', 'state']
    assert ts.observation['image'].shape == (64, 64, 3) and ts.observation['ego'].shape == (48, 48, 3)
    assert ts.observation['video'].shape == (96, 96, 3)
    ts = env.step(np.zeros(2))
    assert [ts.observation[k].shape for k in ('image', 'ego', 'video')] == [(64, 64, 3), (48, 48, 3), (96, 96, 3)]
    assert list(env.observation()) == ['image', 'ego', 'video', 'state']
    assert set(env.observation_spec()) == {'image', 'ego', 'video'}
    g = gym_wrapper.GymWrapper(environment.Environment(**views_zoo.get_config(0)))
    assert set(g.observation_space.spaces) == {'image', 'ego', 'video'}
    obs = g.reset()
    assert [obs[k].shape for k in ('image', 'ego', 'video')] == [(64, 64, 3), (48, 48, 3), (96, 96, 3)]
    env.close()


def test_no_renderer_steps_like_a_renderer():
    """A RawState-only config: reward / discount / step_type equal those of the same config run with a renderer; its
    observation holds only the RawState entry; a render call on the engine fails cleanly."""
    import ctypes
    import torch
    from moog import _engine
    n = 128
    acts = _actions(n, 220)
    bare = _env(views_zoo.get_config(3), n, seed=2)
    full = _env(views_zoo.get_config(0), n, seed=2)
    a, b = bare.reset(), full.reset()
    assert list(a.observation) == ['state']
    for t in range(220):
        a, b = bare.step(acts[t]), full.step(acts[t])
        assert torch.equal(a.step_type, b.step_type), t
        assert torch.equal(a.reward.nan_to_num(-7.0), b.reward.nan_to_num(-7.0)), t
        assert torch.equal(a.discount.nan_to_num(-7.0), b.discount.nan_to_num(-7.0)), t
    assert torch.equal(bare.state_f64, full.state_f64) and torch.equal(bare.state_i32, full.state_i32)
    assert list(bare.observation()) == ['state']
    img = torch.zeros((n, 8, 8, 3), dtype=torch.uint8, device=bare.device)
    rc = bare._lib.moog_engine_render(bare._handle, ctypes.c_void_p(img.data_ptr()), bare._stream())
    assert rc == -1 and b'draws no frames' in bare._lib.moog_last_error()
    with pytest.raises(_engine.EngineError):
        bare.raster_path()
    bare.close()
    full.close()


def test_sub_batches_keep_raw_state_entries():
    cfg = views_zoo.get_config(0)
    env = _env(cfg, 64, seed=1, sub_batches=2)
    ts = env.reset()
    assert list(ts.observation) == ['image', 'ego', 'video', 'state']
    one = _env(cfg, 64, seed=1)
    ref = one.reset()
    import torch
    assert torch.equal(ts.observation['state'].f64, ref.observation['state'].f64)
    a, b = ts.observation['state'].sprites(5), ref.observation['state'].sprites(5)
    assert list(a) == list(b) and [len(v) for v in a.values()] == [len(v) for v in b.values()]
    bare = _env(views_zoo.get_config(3), 64, seed=1, sub_batches=2)
    assert list(bare.reset().observation) == ['state']
    for e in (env, one, bare):
        e.close()


def test_simulation_environment_returns_every_view():
    from moog import environment
    from moog.env_wrappers import simulation
    env = simulation.SimulationEnvironment(environment.Environment(**views_zoo.get_config(0)))
    ts = env.reset()
    assert list(ts.observation) == ['image', 'ego', 'video', 'state']
    sim = env.sim_step(np.zeros(2))
    assert list(sim.observation) == ['image', 'ego', 'video', 'state']
    assert [sim.observation[k].shape for k in ('image', 'ego', 'video')] == [(64, 64, 3), (48, 48, 3), (96, 96, 3)]
    env.sim_pop()
    obs = env.observation()   # every view redrawn from the restored state
    for k, v in zip(('image', 'ego', 'video'), (ts.observation['image'], ts.observation['ego'], ts.observation['video'])):
        assert np.array_equal(obs[k], v), k
    ts2 = env.step(np.zeros(2))
    assert list(ts2.observation) == ['image', 'ego', 'video', 'state']
    env.close()
