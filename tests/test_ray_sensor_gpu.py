"""RaySensor observer on the MI355X: the readings the ray-sensor kernel writes (include/moog_engine.h moog_engine_add_sensor;
csrc/moog_ray_sensor.hip) against the host model of the same header over the engine's own records, bit for bit, and against
the independent numpy implementation over the reference's recordings; a fan that follows the origin's angle within the
rays the device's own cos / sin may decide differently; planted known answers; action repeat and auto-reset, sub-batches,
facades, re-sized layers, the engine's refusals; and that an engine with a sensor computes what one without it computes."""
import ctypes

import numpy as np
import pytest

import helpers
import test_ray_sensor_host as host
from moog import _abi, _engine, observers
from moog_demos import example_configs

pytestmark = pytest.mark.gpu
FOLLOW = _abi.MOOG_SENSOR_FOLLOW_ANGLE


def _cfg(name, extra, alone=False):
    cfg = example_configs.load(name)
    obs = {} if alone else {k: o for k, o in cfg['observers'].items() if not isinstance(o, observers.RaySensor)}
    obs.update(extra)
    cfg['observers'] = obs
    return cfg


def _env(name, n, extra, seed=0, alone=False, sub_batches=None, **kw):
    from moog import environment
    kw.setdefault('layer_capacity', example_configs.capacity(name))
    cfg = _cfg(name, extra, alone)
    if sub_batches:
        return environment.SubBatchedEnvironment(num_envs=n, sub_batches=sub_batches, seed=seed, **cfg, **kw)
    return environment.BatchedEnvironment(num_envs=n, seed=seed, **cfg, **kw)


def records(env):
    import torch
    torch.cuda.synchronize()
    return env.state_f64.cpu().numpy(), env.state_i32.cpu().numpy()


def check_sensors(env, obs, where):
    """Every sensor of the env without follow_angle: the model's bits over the records the tensors were cast from."""
    c = env.compiled
    f, q = records(env)
    sel = [(k, T) for k, T in c.sensors if not T.flags & FOLLOW]
    want = host.model_cast(host.build_model(), c.program, [T for _, T in sel], f, q)
    for (key, T), w in zip(sel, want):
        g = obs[key].cpu().numpy()
        assert tuple(g.shape) == (f.shape[0], T.n_rays, 2), (where, key)
        print('%s %s: %d readings, %d differ, %d hits' % (where, key, g.size, int((host.bits(g) != host.bits(w)).sum()),
                                                         int((w[:, :, 1] != 0).sum())))
        assert host.same_bits(g, w), (where, key, np.argwhere(host.bits(g) != host.bits(w))[:5])


def four_sensors(origin, num_rays, **kw):
    return {'%s%d' % (mode[0], 16 if dtype == 'float16' else 32):
            observers.RaySensor(origin, num_rays=num_rays, mode=mode, dtype=dtype, max_range=1.5,
                                visible_only=(mode == 'instance'), **kw)
            for mode in ('instance', 'layer') for dtype in ('float32', 'float16')}


@pytest.mark.parametrize('n', [3, 67])
@pytest.mark.parametrize('num_rays', [1, 7, 64, 65, 256])
def test_bit_for_bit_against_the_model(n, num_rays):
    """ray_zoo, both modes and both dtypes on one handle: after reset(), after each of 8 random steps, and in an
    observation() after a position was edited through env.field()."""
    import torch
    sensors = four_sensors('agent', num_rays)
    env = _env('ray_zoo', n, sensors, seed=2)
    spec = env.observation_spec()
    assert spec['i32'].shape == (num_rays, 2) and spec['l16'].dtype == np.float16 and 'image' in spec and 'table' in spec
    ts = env.reset()
    held = {k: ts.observation[k] for k in sensors}
    check_sensors(env, ts.observation, 'reset')
    torch.manual_seed(1)
    for t in range(8):
        ts = env.step(env.random_action())
        for k in sensors:   # allocated once, rewritten in place
            assert ts.observation[k] is held[k] and ts.observation[k].data_ptr() == held[k].data_ptr()
        check_sensors(env, ts.observation, 'step %d' % t)
    a = env.compiled.layer_slots['agent'][0]
    env.field('position')[:, a, 0] += 0.0625
    check_sensors(env, env.observation(), 'observation')
    assert np.array_equal(env.ray_directions('i32'), sensors['i32'].directions)
    assert len(env.ray_rows('i32')) == env.layout.S and env.ray_rows('i32') == env.table_rows('table')
    env.close()


def test_more_edges_than_one_chunk():
    """falling_balls_64 at 5 envs: 60 balls and 4 walls, more edges per env than one LDS chunk holds; and sub-batches whose
    second part's float16 rays start at an odd ray of the whole tensor."""
    import torch
    o = host.origin_layer_of('falling_balls_64')
    sensors = four_sensors(o, 33)
    env = _env('falling_balls_64', 5, sensors, seed=2)
    ts = env.reset()
    f, q = records(env)
    L, S = env.layout, env.layout.S
    live = (q[:, L.o_flags:L.o_flags + S] & _abi.MOOG_F_ALIVE) != 0
    assert int((q[:, L.o_nverts:L.o_nverts + S] * live).sum(axis=1).max()) > host.build_model().rs_model_chunk()
    check_sensors(env, ts.observation, 'reset')
    torch.manual_seed(1)
    for t in range(4):
        ts = env.step(env.random_action())
        check_sensors(env, ts.observation, 'step %d' % t)
    env.close()
    parts = _env('falling_balls_64', 6, four_sensors(o, 7), seed=2, sub_batches=2)
    assert (6 // 2 * 7) % 2 == 1
    ts = parts.reset()
    check_sensors(parts, ts.observation, 'parts reset')
    ts = parts.step(parts.random_action())
    check_sensors(parts, ts.observation, 'parts step')
    parts.close()


def test_follow_angle_within_the_excused_rays():
    """The device rotates by its own cos / sin, the model by numpy's: every ray whose id an angle change of 1e-12 rad does not
    flip has the model's id and a distance within 1e-6 * max_range of the model's; at most 1 % of the rays are excused."""
    import torch
    sensors = {'f': observers.RaySensor('agent', num_rays=64, follow_angle=True, max_range=1.5),
               'g': observers.RaySensor('agent', num_rays=16, fov=np.pi / 2, follow_angle=True, max_range=0.75, mode='layer',
                                        visible_only=False)}
    env = _env('ray_zoo', 64, sensors, seed=7)
    ts = env.reset()
    torch.manual_seed(5)
    n_ex = n_all = n_bits = 0
    for t in range(4):
        ts = env.step(env.random_action())
        f, q = records(env)
        T = [t_ for _, t_ in env.compiled.sensors]
        ex, base = host.excused_rays(host.build_model(), env.compiled, T, f, q)
        for k, (key, t_) in enumerate(env.compiled.sensors):
            g = ts.observation[key].cpu().numpy()
            keep = ~ex[k]
            assert np.array_equal(g[:, :, 1][keep], base[k][:, :, 1][keep]), (t, key)
            err = np.abs(g[:, :, 0].astype(np.float64) - base[k][:, :, 0].astype(np.float64))[keep]
            assert err.max() <= 1e-6 * t_.max_range, (t, key, err.max())
            n_ex, n_all = n_ex + int(ex[k].sum()), n_all + ex[k].size
            n_bits += int((host.bits(g) != host.bits(base[k])).sum())
    print('follow_angle: %d of %d rays excused; %d readings differ in some bit from the model fed numpy cos / sin' % (n_ex, n_all, n_bits))
    assert n_ex <= 0.01 * n_all
    env.close()


def test_planted_known_answers_on_the_device():
    import torch
    c0 = host.compile_with('ray_zoo', {})
    cases = host.planted_cases(c0)
    env = _env('ray_zoo', len(cases), {}, seed=1)
    assert bytes(env.compiled.program) == bytes(c0.program)
    env.reset()
    variants = [{}, dict(max_range=0.5), dict(max_range=0.75), dict(visible_only=False)]
    assert all(kw in variants for _, _, _, kw, _ in cases)
    lib, bufs, T = env._lib, [], []
    for kw in variants:
        t = host.planted_sensor(c0, **kw)
        idx = ctypes.c_int32()
        _engine.check(lib, lib.moog_engine_add_sensor(env._handle, ctypes.byref(t), ctypes.byref(idx)))
        buf = torch.zeros((len(cases), t.n_rays, 2), dtype=torch.float32, device=env.device)
        _engine.check(lib, lib.moog_engine_set_sensor_buffer(env._handle, idx.value, ctypes.c_void_p(buf.data_ptr())))
        bufs.append(buf)
        T.append(t)
    env.state_f64.copy_(torch.from_numpy(np.stack([f for _, f, _, _, _ in cases])))
    env.state_i32.copy_(torch.from_numpy(np.stack([q for _, _, q, _, _ in cases])))
    _engine.check(lib, lib.moog_engine_observe_sensors(env._handle, env._stream()))
    f, q = records(env)
    want = host.model_cast(host.build_model(), c0.program, T, f, q)
    for k in range(len(variants)):
        assert host.same_bits(bufs[k].cpu().numpy(), want[k]), k
    for e, (name, _, _, kw, answers) in enumerate(cases):
        k = variants.index(kw)
        host.check_planted(name, bufs[k][e].cpu().numpy(), answers, T[k])
    env.close()


@pytest.mark.parametrize('name', ['colliding_predators_32', 'rules_zoo_l1'])
def test_teacher_forced_against_the_recordings(name):
    """Env t holds the reference's state of recorded call t: observation() equals the numpy implementation's readings."""
    import torch
    sensors = host.recording_sensors(name)
    fx = helpers.fixture(name, 0)
    n = len(fx['step_type'])
    env = _env(name, n, sensors)
    c = env.compiled
    _, f64, i32 = host.fixture_records(name, c)
    env.state_f64.copy_(torch.from_numpy(f64))
    env.state_i32.copy_(torch.from_numpy(i32))
    obs = env.observation()
    for key, T in c.sensors:
        want = host.numpy_cast(c, T, f64, i32)
        g = obs[key].cpu().numpy()
        print('%s %s: %d readings, %d differ' % (name, key, g.size, int((host.bits(g) != host.bits(want)).sum())))
        assert host.same_bits(g, want), (name, key)
    env.close()


def test_action_repeat_and_auto_reset():
    """pong, 16 envs, action_repeat=4, across natural episode ends and forced ones: the reading after a call is the reading of
    the record after that call."""
    o = host.origin_layer_of('pong')
    sensors = {'s': observers.RaySensor(o, num_rays=24, max_range=2.0), 'h': observers.RaySensor(o, num_rays=9, mode='layer', dtype='float16')}
    n, k = 16, 4
    env = _env('pong', n, sensors, seed=3, action_repeat=k)
    ts = env.reset()
    check_sensors(env, ts.observation, 'reset')
    rs = np.random.RandomState(0)
    seen_last = seen_first = False
    for call in range(24):
        if call == 2:
            env.state_i32[1::4, env.layout.o_reset_next] = 1
        ts = env.step(rs.uniform(-1, 1, size=(n, 2)))
        check_sensors(env, ts.observation, 'call %d' % call)
        st = ts.step_type.cpu().numpy()
        seen_last |= bool((st == 2).any()) and call > 2
        seen_first |= bool((st == 0).any()) and call > 3
    assert seen_last and seen_first, 'no episode ended by itself: the run is too short to show an auto-reset'
    env.close()


def test_sub_batches_facades_and_spaces():
    """The demo config as it is (a table, a fixed fan, a float16 fan that follows the angle): sub-batches equal the whole
    batch, the single-env facade hands out env 0's arrays, GymWrapper a Box."""
    import torch
    from moog import environment
    from moog.env_wrappers import gym_wrapper
    n = 6
    kw = dict(layer_capacity=example_configs.capacity('ray_zoo'), seed=5)
    whole = environment.BatchedEnvironment(num_envs=n, **example_configs.load('ray_zoo'), **kw)
    parts = environment.SubBatchedEnvironment(num_envs=n, sub_batches=2, **example_configs.load('ray_zoo'), **kw)
    keys = ('rays', 'front')
    a, b = whole.reset(), parts.reset()
    rs = np.random.RandomState(1)
    for t in range(6):
        torch.cuda.synchronize()
        for key in keys:
            assert b.observation[key] is parts.tables[key] and tuple(b.observation[key].shape) == tuple(a.observation[key].shape)
            assert host.same_bits(b.observation[key].cpu().numpy(), a.observation[key].cpu().numpy()), (t, key)
        check_sensors(whole, a.observation, 'whole %d' % t)
        act = torch.from_numpy(rs.uniform(-1, 1, size=(n, 2))).to(whole.device)
        a, b = whole.step(act), parts.step(act)
    assert parts.observation_spec()['front'].shape == (16, 2) and parts.ray_rows('rays') == whole.ray_rows('rays')
    assert np.array_equal(parts.ray_directions('front'), whole.ray_directions('front'))
    whole.close()
    parts.close()
    single = environment.Environment(layer_capacity=example_configs.capacity('ray_zoo'), seed=5, **example_configs.load('ray_zoo'))
    ts = single.reset()
    ref = environment.BatchedEnvironment(num_envs=1, **example_configs.load('ray_zoo'), **kw)
    want = ref.reset().observation
    for key in keys:
        got = ts.observation[key]
        assert isinstance(got, np.ndarray) and got.shape == tuple(want[key].shape[1:]) and got.dtype == want[key].cpu().numpy().dtype
        assert host.same_bits(got, want[key][0].cpu().numpy())
        assert host.same_bits(single.observation()[key], got)
    ref.close()
    gym = gym_wrapper.GymWrapper(single)
    space = gym.observation_space
    assert space['rays'].shape == (32, 2) and space['rays'].dtype == np.float32
    assert space['front'].shape == (16, 2) and space['front'].dtype == np.float16 and space['image'].dtype == np.uint8
    obs, reward, done, info = gym.step(np.array([0.1, -0.2]))
    assert obs['rays'].shape == (32, 2)
    single.close()


def test_fitted_layers_change_the_row_ids():
    import torch
    sensors = {'s': observers.RaySensor('agent', layers=('prey', 'shapes', 'walls'), max_range=1.5),
               'l': observers.RaySensor('agent', num_rays=9, layers=('prey', 'walls'), mode='layer', dtype='float16')}
    env = _env('ray_zoo', 8, sensors, seed=6, layer_capacity={'prey': 20})
    ts = env.reset()
    torch.manual_seed(2)
    for t in range(6):
        ts = env.step(env.random_action())
    check_sensors(env, ts.observation, 'before')
    rows_before = env.ray_rows('s')
    caps = env.fit_layer_capacity()
    assert caps and caps['prey'] < 20
    obs = env._observation()
    rows = env.ray_rows('s')   # the rows, and with them the ids of `shapes` and `walls`, moved; the readings are under the new ids
    assert len(rows) == len(rows_before) - (20 - caps['prey']) and rows.index(('shapes', 0)) == caps['prey']
    assert obs['s'] is env.tables['s'] and dict(env.compiled.sensors)['s'].n_rows == len(rows)
    check_sensors(env, obs, 'fitted')
    assert int((obs['s'][:, :, 1] > caps['prey']).sum()) > 0
    for t in range(3):   # (the fitted layer has room for at least four more)
        ts = env.step(env.random_action())
        check_sensors(env, ts.observation, 'after %d' % t)
    env.close()


def test_engine_refuses_bad_sensors():
    env = _env('ray_zoo', 2, {'s%d' % k: observers.RaySensor('agent') for k in range(_abi.MOOG_MAX_SENSORS)})
    lib, idx = env._lib, ctypes.c_int32()
    good = dict(env.compiled.sensors)['s0']
    assert lib.moog_engine_add_sensor(env._handle, ctypes.byref(good), ctypes.byref(idx)) == _abi.MOOG_E_INVALID   # a fifth
    assert b'MOOG_MAX_SENSORS' in lib.moog_last_error()
    env.close()
    env = _env('ray_zoo', 2, {})
    S = env.layout.S
    for edit, word in ((lambda T: setattr(T, 'n_rays', 257), b'n_rays'), (lambda T: setattr(T, 'n_rays', 0), b'n_rays'),
                       (lambda T: setattr(T, 'max_range', float('inf')), b'max_range'), (lambda T: setattr(T, 'max_range', -1.0), b'max_range'),
                       (lambda T: (setattr(T, 'max_range', 70000.0), setattr(T, 'dtype', _abi.MOOG_TABLE_F16)), b'65504'),
                       (lambda T: setattr(T, 'mode', 7), b'mode'), (lambda T: setattr(T, 'dtype', 7), b'dtype'),
                       (lambda T: setattr(T, 'origin_slot', S), b'origin'), (lambda T: T.row_slot.__setitem__(0, S), b'slot'),
                       (lambda T: T.row_slot.__setitem__(1, T.row_slot[0]), b'two rows'),
                       (lambda T: T.dirs[5].__setitem__(0, float('nan')), b'direction')):
        T = _abi.Sensor.from_buffer_copy(good)
        edit(T)
        assert lib.moog_engine_add_sensor(env._handle, ctypes.byref(T), ctypes.byref(idx)) == _abi.MOOG_E_INVALID
        assert word in lib.moog_last_error(), (word, lib.moog_last_error())
    assert lib.moog_engine_set_sensor_buffer(env._handle, 0, None) == _abi.MOOG_E_INVALID   # (no sensor was added)
    _engine.check(lib, lib.moog_engine_observe_sensors(env._handle, env._stream()))          # nothing bound: nothing to do
    env.reset()
    env.close()


def test_one_bracket_per_call():
    """A table and two sensors on one handle: MOOG_K_TABLES counts one per reset / step call."""
    from moog import environment
    import torch
    env = environment.BatchedEnvironment(num_envs=4, seed=1, layer_capacity=example_configs.capacity('ray_zoo'),
                                         **example_configs.load('ray_zoo'))
    assert len(env.compiled.tables) == 1 and len(env.compiled.sensors) == 2
    env.set_timing(True, kernels=[_abi.MOOG_K_TABLES])
    env.reset()
    torch.manual_seed(1)
    for t in range(8):
        env.step(env.random_action())
    assert env.kernel_time(_abi.MOOG_K_TABLES)[1] == 9
    env.close()


def test_nothing_else_moved():
    """colliding_predators_32 at 32 envs with a sensor beside the PILRenderer and without: after 8 calls the time steps, the
    frames and the records are equal, and both engines step and draw with the same kernels."""
    import torch
    o = host.origin_layer_of('colliding_predators_32')
    plain = _env('colliding_predators_32', 32, {}, seed=9)
    sens = _env('colliding_predators_32', 32, {'s': observers.RaySensor(o, max_range=2.0)}, seed=9)
    assert bytes(plain.compiled.program) == bytes(sens.compiled.program)
    assert plain.step_kernel() == sens.step_kernel() and plain.raster_path() == sens.raster_path()
    assert plain.kernel_variant == sens.kernel_variant
    a, b = plain.reset(), sens.reset()
    rs = np.random.RandomState(2)
    for t in range(8):
        act = rs.uniform(-1, 1, size=(32, 2))
        a, b = plain.step(act), sens.step(act)
        torch.cuda.synchronize()
        for x, y in ((a.step_type, b.step_type), (a.reward, b.reward), (a.discount, b.discount),
                     (a.observation['image'], b.observation['image']), (plain.state_i32, sens.state_i32)):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True), t
        assert np.array_equal(plain.state_f64.cpu().numpy().view(np.uint64), sens.state_f64.cpu().numpy().view(np.uint64)), t
    check_sensors(sens, b.observation, 'last')
    assert plain.step_kernel() == sens.step_kernel() and plain.raster_path() == sens.raster_path()
    assert list(a.observation) == ['image'] and list(b.observation) == ['image', 's']
    plain.close()
    sens.close()
