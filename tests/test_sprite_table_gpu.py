"""SpriteTable observer on the MI355X: the tables the sprite-table kernel writes (include/moog_engine.h
moog_engine_add_table; csrc/moog_sprite_table.hip) against numpy's cast of the engine's own records and of the reference's
recordings, bit for bit; action repeat and auto-reset, sub-batches, facades, re-sized layers; and that an engine with a
table computes what one without it computes."""
import ctypes

import numpy as np
import pytest

import helpers
import test_sprite_table_host as host
from moog import _abi, _engine, observers
from moog_demos import example_configs

pytestmark = pytest.mark.gpu
ALL = observers.SpriteTable.ALL_COLUMNS


def _cfg(name, tables, alone=False):
    cfg = example_configs.load(name)
    obs = {} if alone else dict(cfg['observers'])
    obs.update(tables)
    cfg['observers'] = obs
    return cfg


def _env(name, n, tables, seed=0, alone=False, sub_batches=None, **kw):
    from moog import environment
    kw.setdefault('layer_capacity', example_configs.capacity(name))
    cfg = _cfg(name, tables, alone)
    if sub_batches:
        return environment.SubBatchedEnvironment(num_envs=n, sub_batches=sub_batches, seed=seed, **cfg, **kw)
    return environment.BatchedEnvironment(num_envs=n, seed=seed, **cfg, **kw)


def expected(env, key):
    """The table `key` from the engine's own records, read back from the same tensors and cast by numpy."""
    import torch
    torch.cuda.synchronize()
    c = env.compiled
    P, L, S = c.program, c.layout, c.layout.S
    f, q = env.state_f64.cpu().numpy(), env.state_i32.cpu().numpy()
    T = dict(c.tables)[key]
    two = lambda o, k: f[:, o:o + 2 * S].reshape(-1, S, 2)[:, :, k]
    col3 = lambda k: f[:, L.o_color:L.o_color + 3 * S].reshape(-1, S, 3)[:, :, k]
    one = lambda o: f[:, o:o + S]
    alive = (q[:, L.o_flags:L.o_flags + S] & _abi.MOOG_F_ALIVE) != 0
    src = {'x': lambda: two(L.o_pos, 0), 'y': lambda: two(L.o_pos, 1), 'x_vel': lambda: two(L.o_vel, 0),
           'y_vel': lambda: two(L.o_vel, 1), 'angle': lambda: one(L.o_angle), 'angle_vel': lambda: one(L.o_angvel),
           'mass': lambda: one(L.o_mass), 'c0': lambda: col3(0), 'c1': lambda: col3(1), 'c2': lambda: col3(2),
           'scale': lambda: one(L.o_scale), 'aspect_ratio': lambda: one(L.o_aspect),
           'opacity': lambda: q[:, L.o_opacity:L.o_opacity + S], 'shape_id': lambda: q[:, L.o_shape:L.o_shape + S],
           'n_vertices': lambda: q[:, L.o_nverts:L.o_nverts + S], 'alive': lambda: alive,
           'layer': lambda: np.broadcast_to(np.array([P.slot_layer[s] for s in range(S)]), alive.shape)}
    slots = [T.row_slot[r] for r in range(T.n_rows)]
    dt = host.sprite_table.table_dtype(T)
    out = np.zeros((f.shape[0], T.n_rows, T.n_cols), dt)
    with np.errstate(all='ignore'):
        for k, name in enumerate(env.table_columns(key)):
            out[:, :, k] = np.where(alive[:, slots], np.asarray(src[name]())[:, slots].astype(dt), dt.type(0))
    return out


def check_tables(env, obs, where):
    for key, _ in env.compiled.tables:
        got = obs[key]
        want = expected(env, key)
        assert tuple(got.shape) == want.shape, (where, key)
        g = got.cpu().numpy()
        print('%s %s: %d elements, %d differ' % (where, key, g.size, int((host.bits(g) != host.bits(want)).sum())))
        assert host.same_bits(g, want), (where, key, np.argwhere(host.bits(g) != host.bits(want))[:5])


@pytest.mark.parametrize('name,n', [('pong', 3), ('pong', 67), ('falling_balls_64', 5)])
def test_tables_equal_the_cast_of_the_record(name, n):
    import torch
    tables = {'t32': observers.SpriteTable(), 't16': observers.SpriteTable(dtype='float16')}
    env = _env(name, n, tables, seed=2)
    if name == 'falling_balls_64':   # (64 slots: 4 walls and 60 balls -- several workgroups' worth of elements per env)
        assert dict(env.compiled.tables)['t32'].n_rows == 64
    spec = env.observation_spec()
    assert spec['t32'].shape == tuple(env.tables['t32'].shape[1:]) and spec['t16'].dtype == np.float16 and 'image' in spec
    env.set_timing(True, kernels=[_abi.MOOG_K_TABLES])
    ts = env.reset()
    held = {k: ts.observation[k] for k in tables}
    check_tables(env, ts.observation, 'reset')
    torch.manual_seed(1)
    for t in range(8):
        ts = env.step(env.random_action())
        for k in tables:   # allocated once, rewritten in place
            assert ts.observation[k] is held[k] and ts.observation[k].data_ptr() == held[k].data_ptr()
        check_tables(env, ts.observation, 'step %d' % t)
    assert env.kernel_time(_abi.MOOG_K_TABLES)[1] == 9   # one launch per call, whatever the number of tables
    assert len(env.table_rows('t32')) == env.tables['t32'].shape[1] and env.table_columns('t16') == observers.SpriteTable.DEFAULT_COLUMNS
    env.close()


@pytest.mark.parametrize('alone', [False, True])
def test_two_tables_on_one_handle(alone):
    """Tables of different layers, columns and dtypes on one handle (one launch), a float16 table whose rows x columns is
    odd; beside the config's PILRenderer and with no renderer at all (a program that draws no frames)."""
    import torch
    tables = {'odd16': observers.SpriteTable(layers=('agent', 'predators'), columns=('x', 'scale', 'alive'), dtype='float16'),
              'all32': observers.SpriteTable(columns=ALL),
              'state': observers.RawState()}
    env = _env('rules_zoo_l1', 5, tables, seed=4, alone=alone, keep_sprite_factors=True)
    T = dict(env.compiled.tables)
    assert (T['odd16'].n_rows * T['odd16'].n_cols) % 2 == 1 and (5 * T['odd16'].n_rows * T['odd16'].n_cols) % 2 == 1
    R = env.compiled.program.render
    assert ((R.width, R.height) == (0, 0)) == alone and (env.compiled.observer_key is None) == alone
    ts = env.reset()
    assert ('image' in ts.observation) != alone
    check_tables(env, ts.observation, 'reset')
    torch.manual_seed(3)
    for t in range(8):
        ts = env.step(env.random_action())
        check_tables(env, ts.observation, 'step %d' % t)
    env.state_f64[:, env.layout.o_pos] += 0.25   # observation(): the records as they are now
    check_tables(env, env.observation(), 'observation')
    env.close()


def test_engine_refuses_bad_tables():
    env = _env('pong', 2, {f't{k}': observers.SpriteTable() for k in range(_abi.MOOG_MAX_TABLES)})
    lib, idx = env._lib, ctypes.c_int32()
    good = dict(env.compiled.tables)['t0']
    assert lib.moog_engine_add_table(env._handle, ctypes.byref(good), ctypes.byref(idx)) == _abi.MOOG_E_INVALID   # a fifth
    assert b'MOOG_MAX_TABLES' in lib.moog_last_error()
    env.close()
    env = _env('pong', 2, {})
    for edit, word in ((lambda T: T.row_slot.__setitem__(0, env.layout.S), b'slot'),
                       (lambda T: T.cols.__setitem__(0, _abi.MOOG_TCOL_SCALE), b'o_scale'),
                       (lambda T: setattr(T, 'n_cols', 0), b'n_cols')):
        T = _abi.Table.from_buffer_copy(good)
        edit(T)
        assert lib.moog_engine_add_table(env._handle, ctypes.byref(T), ctypes.byref(idx)) == _abi.MOOG_E_INVALID
        assert word in lib.moog_last_error()
    assert lib.moog_engine_set_table_buffer(env._handle, 0, None) == _abi.MOOG_E_INVALID   # (no table was added)
    _engine.check(lib, lib.moog_engine_observe_tables(env._handle, env._stream()))          # nothing bound: nothing to do
    env.reset()
    env.close()


@pytest.mark.parametrize('name', ['colliding_predators_32', 'rules_zoo_l1'])
def test_teacher_forced_against_the_reference(name):
    """Env t holds the reference's state of recorded call t: observation() equals the recording's attributes cast by numpy."""
    import torch
    tables = {'d32': observers.SpriteTable(), 'a16': observers.SpriteTable(columns=ALL, dtype='float16')}
    fx = helpers.fixture(name, 0)
    n = len(fx['step_type'])
    env = _env(name, n, tables, keep_sprite_factors=True)
    c = env.compiled
    _, f64, i32 = host.fixture_records(name, c)
    env.state_f64.copy_(torch.from_numpy(f64))
    env.state_i32.copy_(torch.from_numpy(i32))
    obs = env.observation()
    for key, T in c.tables:
        want = host.expected_from_fixture(fx, c, T, tables[key].columns, list(range(c.layout.S)))
        g = obs[key].cpu().numpy()
        print('%s %s: %d elements, %d differ' % (name, key, g.size, int((host.bits(g) != host.bits(want)).sum())))
        assert host.same_bits(g, want), (name, key)
    if name == 'rules_zoo_l1':   # row i of an appended layer is the reference's i-th sprite: after creations (16), after a purge (17)
        g = obs['d32'].cpu().numpy()
        rows = env.table_rows('d32')
        for layer in ('predators', 'prey'):
            s0, cap = c.layer_slots[layer]
            r0 = rows.index((layer, 0))
            assert rows[r0:r0 + cap] == [(layer, k) for k in range(cap)]
            for t in (16, 17):
                live = int(fx['alive'][t, s0:s0 + cap].sum())
                assert np.all(fx['alive'][t, s0:s0 + live] == 1)   # (the reference's list, packed at the front)
                for i in range(live):
                    assert g[t, r0 + i, 0] == 1 and g[t, r0 + i, 1] == np.float32(fx['pos'][t, s0 + i, 0])
                assert np.all(g[t, r0 + live:r0 + cap] == 0)
        assert int(fx['alive'][16, c.layer_slots['predators'][0]:][:8].sum()) == 2
        assert int(fx['alive'][17, c.layer_slots['predators'][0]:][:8].sum()) == 0
    env.close()


def test_one_rounding_on_the_device():
    vals = np.array([1 + 2.0 ** -11 + 2.0 ** -30, 65519.999, 3 * 2.0 ** -24, np.nan, np.inf, 65520.0, -(1 + 2.0 ** -11 - 2.0 ** -30),
                     2.0 ** -25, np.nextafter(2.0 ** -25, 1)])
    tables = {'h': observers.SpriteTable(columns=('x', 'alive'), dtype='float16'), 's': observers.SpriteTable(columns=('x',))}
    env = _env('colliding_predators_32', 2, tables, alone=True)   # (no renderer: nothing draws the sprites put at NaN and inf)
    env.reset()
    import torch
    live = env.field('alive')[0].nonzero().flatten()[:len(vals)]
    assert len(live) == len(vals)
    env.field('position')[0, live, 0] = torch.from_numpy(vals).to(env.device)
    obs = env.observation()
    rows = live.cpu().numpy()   # (every layer, in order: row = slot)
    with np.errstate(all='ignore'):
        want16, want32 = vals.astype(np.float16), vals.astype(np.float32)
    got16, got32 = obs['h'][0].cpu().numpy()[rows, 0], obs['s'][0].cpu().numpy()[rows, 0]
    print('float16 got', got16, 'want', want16)
    assert host.same_bits(got16, want16) and host.same_bits(got32, want32)
    assert float(got16[0]) == 1 + 2.0 ** -10 and np.isinf(got16[5]) and got16[1] == np.float16(65504) and np.isnan(got16[3])
    check_tables(env, obs, 'edited')
    env.close()


def test_action_repeat_and_auto_reset():
    """pong, 16 envs, action_repeat=4, across natural episode ends and forced ones: the table after each call is the cast of the
    record after that call, and an engine making single calls from the same records shows the same table at the env-step
    each env stopped at."""
    import torch
    tables = {'t': observers.SpriteTable(), 'h': observers.SpriteTable(columns=('x', 'y', 'alive'), dtype='float16')}
    n, k = 16, 4
    env = _env('pong', n, tables, seed=3, action_repeat=k)
    one = _env('pong', n, tables, seed=3)
    ts = env.reset()
    check_tables(env, ts.observation, 'reset')
    rs = np.random.RandomState(0)
    seen_last = seen_first = False
    for call in range(24):
        if call == 2:
            env.state_i32[1::4, env.layout.o_reset_next] = 1
        one.state_f64.copy_(env.state_f64)
        one.state_i32.copy_(env.state_i32)
        a = rs.uniform(-1, 1, size=(n, 2))
        ts = env.step(a)
        check_tables(env, ts.observation, 'call %d' % call)
        singles = []
        for _ in range(k):
            o = one.step(a).observation
            singles.append({key: o[key].cpu().numpy().copy() for key in tables})
        m = env.repeat_count.cpu().numpy()
        st = ts.step_type.cpu().numpy()
        assert np.all((m == 0) == (st == 0)) and np.all(m <= k)
        for key in tables:
            got = ts.observation[key].cpu().numpy()
            for i in range(n):
                assert host.same_bits(got[i], singles[max(1, int(m[i])) - 1][key][i]), (call, key, i, int(m[i]))
        seen_last |= bool((st == 2).any()) and call > 2
        seen_first |= bool((st == 0).any()) and call > 3
    assert seen_last and seen_first, 'no episode ended by itself: the run is too short to show an auto-reset'
    env.close()
    one.close()


def test_sub_batches_facades_and_spaces():
    import torch
    from moog import environment
    from moog.env_wrappers import gym_wrapper
    tables = {'t': observers.SpriteTable(), 'h': observers.SpriteTable(layers=('agent', 'predators'), columns=('x', 'y', 'alive'), dtype='float16')}
    n = 6
    whole = _env('rules_zoo_l1', n, tables, seed=5)
    parts = _env('rules_zoo_l1', n, tables, seed=5, sub_batches=2)
    per_env = parts.tables['h'].shape[1] * parts.tables['h'].shape[2]
    assert (n // 2 * per_env) % 2 == 1   # the second part's float16 slice starts in the middle of a dword
    a, b = whole.reset(), parts.reset()
    rs = np.random.RandomState(1)
    for t in range(6):
        for key in tables:
            torch.cuda.synchronize()
            assert b.observation[key] is parts.tables[key] and tuple(b.observation[key].shape) == tuple(a.observation[key].shape)
            assert host.same_bits(b.observation[key].cpu().numpy(), a.observation[key].cpu().numpy()), (t, key)
        check_tables(whole, a.observation, 'whole %d' % t)
        act = torch.from_numpy(rs.uniform(-1, 1, size=(n, 2))).to(whole.device)
        a, b = whole.step(act), parts.step(act)
    assert parts.observation_spec()['h'].shape == (9, 3) and parts.table_rows('h') == whole.table_rows('h')
    assert parts.table_columns('h') == ('x', 'y', 'alive')
    whole.close()
    parts.close()
    # the single-env facade: env 0's numpy array; GymWrapper: a Box of the table's shape
    cfg = _cfg('rules_zoo_l1', tables)
    single = environment.Environment(layer_capacity=example_configs.capacity('rules_zoo_l1'), seed=5, **cfg)
    ts = single.reset()
    ref = _env('rules_zoo_l1', 1, tables, seed=5)
    want = ref.reset().observation
    for key in tables:
        got = ts.observation[key]
        assert isinstance(got, np.ndarray) and got.shape == tuple(want[key].shape[1:]) and got.dtype == want[key].cpu().numpy().dtype
        assert host.same_bits(got, want[key][0].cpu().numpy())
        assert host.same_bits(single.observation()[key], got)
    ref.close()
    gym = gym_wrapper.GymWrapper(single)
    space = gym.observation_space
    assert space['t'].shape == ts.observation['t'].shape and space['t'].dtype == np.float32
    assert space['h'].shape == (9, 3) and space['h'].dtype == np.float16 and space['image'].dtype == np.uint8
    obs, reward, done, info = gym.step(np.array([0.1, -0.2]))
    assert obs['t'].shape == space['t'].shape
    single.close()


def test_fitted_layers_change_the_row_count():
    import torch
    tables = {'t': observers.SpriteTable(), 'h': observers.SpriteTable(layers=('predators', 'prey'), columns=ALL, dtype='float16')}
    env = _env('rules_zoo_l1', 8, tables, seed=6, keep_sprite_factors=True, layer_capacity={'prey': 20, 'predators': 24})
    ts = env.reset()
    before = {k: tuple(ts.observation[k].shape) for k in tables}
    torch.manual_seed(2)
    for t in range(6):
        ts = env.step(env.random_action())
    check_tables(env, ts.observation, 'before')
    caps = env.fit_layer_capacity()
    assert caps and all(v < {'prey': 20, 'predators': 24}[k] for k, v in caps.items())
    obs = env._observation()
    for k in tables:   # re-created with the new row count, and already filled from the records that moved over
        assert tuple(obs[k].shape) != before[k] and obs[k].shape[1] == len(env.table_rows(k)) == env.observation_spec()[k].shape[0]
    check_tables(env, obs, 'fitted')
    for t in range(6):
        ts = env.step(env.random_action())
        check_tables(env, ts.observation, 'after %d' % t)
    env.close()


def test_nothing_else_moved():
    """colliding_predators_32 at 32 envs with a table beside the PILRenderer and without: after 8 calls the time steps, the
    frames and the records are equal, and both engines step and draw with the same kernels."""
    import torch
    plain = _env('colliding_predators_32', 32, {}, seed=9)
    table = _env('colliding_predators_32', 32, {'t': observers.SpriteTable()}, seed=9)
    assert bytes(plain.compiled.program) == bytes(table.compiled.program)
    assert plain.step_kernel() == table.step_kernel() and plain.raster_path() == table.raster_path()
    assert plain.kernel_variant == table.kernel_variant
    a, b = plain.reset(), table.reset()
    rs = np.random.RandomState(2)
    for t in range(8):
        act = rs.uniform(-1, 1, size=(32, 2))
        a, b = plain.step(act), table.step(act)
        torch.cuda.synchronize()
        for x, y in ((a.step_type, b.step_type), (a.reward, b.reward), (a.discount, b.discount),
                     (a.observation['image'], b.observation['image']), (plain.state_i32, table.state_i32)):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True), t
        assert np.array_equal(plain.state_f64.cpu().numpy().view(np.uint64), table.state_f64.cpu().numpy().view(np.uint64)), t
    check_tables(table, b.observation, 'last')
    assert plain.step_kernel() == table.step_kernel() and plain.raster_path() == table.raster_path()
    assert list(a.observation) == ['image'] and list(b.observation) == ['image', 't']
    plain.close()
    table.close()
