"""Contacts observer on the MI355X: the bytes the contacts kernel writes (include/moog_engine.h moog_engine_add_contacts;
csrc/moog_contacts.hip) against the host model of the same header over the engine's own records, byte for byte, and against
the matrices recorded with matplotlib; more candidates than one chunk; planted known answers through the raw ABI; action
repeat and auto-reset, sub-batches, facades, re-sized layers, the engine's refusals, the shared MOOG_K_TABLES bracket; and
that an engine with a contacts observer computes what one without it computes."""
import ctypes

import numpy as np
import pytest

import helpers
import test_contacts_host as host
from moog import _abi, _engine, observers
from moog_demos import example_configs

pytestmark = pytest.mark.gpu


def _cfg(name, extra, alone=False):
    cfg = example_configs.load(name)
    obs = {} if alone else dict(cfg['observers'])
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


def check_contacts(env, obs, where, cands=False):
    """Every contacts observer of the env: the model's bytes over the records the tensors were written from."""
    c = env.compiled
    f, q = records(env)
    want, nc = host.model_observe(host.build_model(), c.program, [T for _, T in c.contacts], f, q, cands=True)
    for (key, T), w in zip(c.contacts, want):
        g = obs[key].cpu().numpy()
        assert g.dtype == np.uint8 and tuple(g.shape) == tuple(w.shape), (where, key, g.shape, w.shape)
        print('%s %s: %d flags, %d differ, %d set' % (where, key, g.size, int((g != w).sum()), int(w.sum())))
        assert np.array_equal(g, w), (where, key, np.argwhere(g != w)[:5])
    return nc if cands else None


def zoo_observers():
    return {k: observers.Contacts(**kw) for k, kw in host.ZOO.items()}


@pytest.mark.parametrize('n', [3, 67])
def test_byte_for_byte_against_the_model(n):
    """ray_zoo, four observers on one handle (pair and layer, square and rectangular, one of 7 x 11 bytes an env): after
    reset(), after each of 8 random steps, and in an observation() after a position was edited through env.field()."""
    import torch
    obs = zoo_observers()
    env = _env('ray_zoo', n, obs, seed=2)
    spec = env.observation_spec()
    assert spec['pair'].shape == (36, 36) and spec['odd'].shape == (7, 11) and spec['layer'].shape == (25, 4)
    assert all(spec[k].dtype == np.uint8 for k in obs) and 'image' in spec and 'table' in spec and 'rays' in spec
    ts = env.reset()
    held = {k: ts.observation[k] for k in obs}
    ptrs = {k: held[k].data_ptr() for k in obs}
    check_contacts(env, ts.observation, 'reset')
    torch.manual_seed(1)
    n_set = 0
    for t in range(8):
        ts = env.step(env.random_action())
        for k in obs:   # allocated once, rewritten in place
            assert ts.observation[k] is held[k] and ts.observation[k].data_ptr() == ptrs[k]
        check_contacts(env, ts.observation, 'step %d' % t)
        n_set += int(ts.observation['pair'].sum())
    assert n_set > 0
    a = env.compiled.layer_slots['agent'][0]
    env.field('position')[:, a, 0] += 0.0625
    check_contacts(env, env.observation(), 'observation')
    rows_0, rows_1 = env.contact_rows('pair')
    assert rows_0 == rows_1 == env.table_rows('table') and len(env.contact_rows('odd')[1]) == 11
    env.close()


def test_more_candidates_than_one_chunk():
    """falling_balls_64 at 5 envs: 64 slots (4 walls, 60 balls), so 'all' is 64 x 64 and 'rect' keeps 60 + 64 rows in LDS --
    more than one lane pass over rows; the balls planted in a cluster so that an env has more candidates past the broad phase
    than one candidate chunk holds."""
    import torch
    names = host.layers_with_slots('falling_balls_64')
    obs = {'all': observers.Contacts(tuple(names)), 'all_l': observers.Contacts(tuple(names), mode='layer'),
           'rect': observers.Contacts(names[-1], tuple(names))}
    env = _env('falling_balls_64', 5, obs, seed=2)
    ts = env.reset()
    assert ts.observation['all'].shape[1:] == (64, 64) and ts.observation['rect'].shape[1:] == (60, 64)
    check_contacts(env, ts.observation, 'reset')
    torch.manual_seed(1)
    for t in range(2):
        ts = env.step(env.random_action())
        check_contacts(env, ts.observation, 'step %d' % t)
    # the cluster: every sprite of envs 1 and 3 moved (vertices with the position) to within a small disc
    f, q = records(env)
    c, L, S = env.compiled, env.layout, env.layout.S
    rs = np.random.RandomState(4)
    for e in (1, 3):
        for s in range(S):
            if not q[e, L.o_flags + s] & _abi.MOOG_F_ALIVE or f[e, L.o_maxr + s] > 0.2:   # (not the walls)
                continue
            new = np.array([0.5, 0.5]) + rs.uniform(-0.04, 0.04, size=2)
            d = new - f[e, L.o_pos + 2 * s:L.o_pos + 2 * s + 2]
            o, nv = L.o_verts + 2 * c.program.slot_voff[s], int(q[e, L.o_nverts + s])
            f[e, o:o + 2 * nv] += np.tile(d, nv)
            f[e, L.o_pos + 2 * s:L.o_pos + 2 * s + 2] = new
    env.state_f64.copy_(torch.from_numpy(f))
    nc = check_contacts(env, env.observation(), 'cluster', cands=True)
    print('candidates past the broad phase per env:', nc[0].tolist())
    assert nc[0].max() > host.build_model().ct_model_chunk()
    env.close()


@pytest.mark.parametrize('name', host.RECORDINGS)
def test_teacher_forced_against_the_recorded_matrices(name):
    """Env t holds the reference's state of recorded call t: observation() equals what matplotlib said, every pair."""
    import torch
    obs = host.recording_observers(name)
    M, counts = host.recorded_matrices(name)
    n = M.shape[0]
    env = _env(name, n, obs)
    c = env.compiled
    _, f64, i32 = host.fixture_records(name, c)
    env.state_f64.copy_(torch.from_numpy(f64))
    env.state_i32.copy_(torch.from_numpy(i32))
    got = env.observation()
    for key, T in c.contacts:
        g = got[key].cpu().numpy()
        want = np.stack([host.expected(c.program, T, M[t]) for t in range(n)])
        print('%s %s: %d flags, %d differ, %d overlaps' % (name, key, g.size, int((g != want).sum()), int(want.sum())))
        assert np.array_equal(g, want), (name, key)
    assert int(got['all'].sum()) == counts[2] == host.COUNTS[name][3]
    env.close()


def test_planted_known_answers_on_the_device():
    """The planted scenes through the raw ABI (the predator slots of colliding_predators_32 hold the polygons of up to 15
    vertices; the model has the 128-vertex ones on its synthetic layout), with a handle-less add first and an unbound observe
    that does nothing."""
    import torch
    env = _env('colliding_predators_32', 12, {}, seed=1)
    c = env.compiled
    lib, idx = env._lib, ctypes.c_int32()
    T0 = host.all_slots(c)
    assert lib.moog_engine_add_contacts(None, ctypes.byref(T0), ctypes.byref(idx)) == _abi.MOOG_E_INVALID
    assert b'null argument' in lib.moog_last_error()
    env.reset()
    descs = [T0, host.all_slots(c, flags=host.VISIBLE), host.all_slots(c, mode=host.LAYER), host.all_slots(c, rows_1=[1, 0, 3, 2])]
    ids = []
    for T in descs:
        _engine.check(lib, lib.moog_engine_add_contacts(env._handle, ctypes.byref(T), ctypes.byref(idx)))
        ids.append(idx.value)
    _engine.check(lib, lib.moog_engine_observe_contacts(env._handle, env._stream()))   # nothing bound: nothing to do
    m = host.build_model()
    bufs = []
    for T, k in zip(descs, ids):
        n0, n1, nl, _ = host.model_shape(m, c.program, T)
        buf = torch.full((12, n0, nl if T.mode == host.LAYER else n1), 0x55, dtype=torch.uint8, device=env.device)
        _engine.check(lib, lib.moog_engine_set_contacts_buffer(env._handle, k, ctypes.c_void_p(buf.data_ptr())))
        bufs.append(buf)
    off = c.layer_slots['predators'][0]   # scene slot s lives in engine slot off + s
    vcap = min(int(c.program.slot_vcap[off + s]) for s in range(4))
    f64, i32, answers = host.planted_scenes(host.synthetic(c, vcap=128))
    small = {e: a for e, a in answers.items() if e not in (9, 11)}   # (scenes 9 and 11 need 128 vertices a slot)
    g64, g32 = host.blank(c, 12)
    sc = host.synthetic(c, vcap=128)
    for e in small:
        for s in range(4):
            nv = int(i32[e, sc.layout.o_nverts + s])
            if i32[e, sc.layout.o_flags + s] or nv:
                assert nv <= vcap
                o = sc.layout.o_verts + 2 * sc.program.slot_voff[s]
                host.plant(c, g64, g32, off + s, f64[e, o:o + 2 * nv].reshape(-1, 2), env=e,
                           pos=f64[e, sc.layout.o_pos + 2 * s:sc.layout.o_pos + 2 * s + 2], maxr=f64[e, sc.layout.o_maxr + s],
                           opacity=int(i32[e, sc.layout.o_opacity + s]), alive=bool(i32[e, sc.layout.o_flags + s]))
    env.state_f64.copy_(torch.from_numpy(g64))
    env.state_i32.copy_(torch.from_numpy(g32))
    _engine.check(lib, lib.moog_engine_observe_contacts(env._handle, env._stream()))
    f, q = records(env)
    want = host.model_observe(m, c.program, descs, f, q)
    for k in range(len(descs)):
        assert np.array_equal(bufs[k].cpu().numpy(), want[k]), k
    g = bufs[0].cpu().numpy()
    for e, ans in small.items():
        for (a, b), v in ans.items():
            assert g[e, off + a, off + b] == v, ('scene %d pair (%d, %d)' % (e, a, b), g[e, off:off + 4, off:off + 4])
    assert g[10, off, off + 1] == 1 and g[10, off + 1, off] == 0
    _engine.check(lib, lib.moog_engine_set_contacts_buffer(env._handle, ids[0], None))
    env.close()


def test_action_repeat_and_auto_reset():
    """pong, 16 envs, action_repeat=4, across natural episode ends and forced ones."""
    names = host.layers_with_slots('pong')
    obs = {'p': observers.Contacts(tuple(names)), 'l': observers.Contacts(names[-1], tuple(names), mode='layer')}
    n, k = 16, 4
    env = _env('pong', n, obs, seed=3, action_repeat=k)
    ts = env.reset()
    check_contacts(env, ts.observation, 'reset')
    rs = np.random.RandomState(0)
    seen_last = seen_first = False
    for call in range(24):
        if call == 2:
            env.state_i32[1::4, env.layout.o_reset_next] = 1
        ts = env.step(rs.uniform(-1, 1, size=(n, 2)))
        check_contacts(env, ts.observation, 'call %d' % call)
        st = ts.step_type.cpu().numpy()
        seen_last |= bool((st == 2).any()) and call > 2
        seen_first |= bool((st == 0).any()) and call > 3
    assert seen_last and seen_first, 'no episode ended by itself: the run is too short to show an auto-reset'
    env.close()


def test_sub_batches_facades_and_spaces():
    """Sub-batches equal the whole batch (the second part of the 7 x 11 tensor starts at an odd byte of it), the single-env
    facade hands out env 0's arrays, GymWrapper a uint8 Box."""
    import torch
    from moog import environment
    from moog.env_wrappers import gym_wrapper
    n = 6
    whole = _env('ray_zoo', n, zoo_observers(), seed=5)
    parts = _env('ray_zoo', n, zoo_observers(), seed=5, sub_batches=2)
    assert (n // 2 * 7 * 11) % 2 == 1
    keys = list(host.ZOO)
    a, b = whole.reset(), parts.reset()
    rs = np.random.RandomState(1)
    for t in range(6):
        torch.cuda.synchronize()
        for key in keys:
            assert b.observation[key] is parts.tables[key] and tuple(b.observation[key].shape) == tuple(a.observation[key].shape)
            assert np.array_equal(b.observation[key].cpu().numpy(), a.observation[key].cpu().numpy()), (t, key)
        check_contacts(whole, a.observation, 'whole %d' % t)
        act = torch.from_numpy(rs.uniform(-1, 1, size=(n, 2))).to(whole.device)
        a, b = whole.step(act), parts.step(act)
    assert parts.parts[1].tables['odd'].data_ptr() % 2 == 1
    assert parts.observation_spec()['odd'].shape == (7, 11) and parts.contact_rows('odd') == whole.contact_rows('odd')
    whole.close()
    parts.close()
    cfg = _cfg('ray_zoo', zoo_observers())
    single = environment.Environment(layer_capacity=example_configs.capacity('ray_zoo'), seed=5, **cfg)
    ts = single.reset()
    ref = _env('ray_zoo', 1, zoo_observers(), seed=5)
    want = ref.reset().observation
    for key in keys:
        got = ts.observation[key]
        assert isinstance(got, np.ndarray) and got.shape == tuple(want[key].shape[1:]) and got.dtype == np.uint8
        assert np.array_equal(got, want[key][0].cpu().numpy())
        assert np.array_equal(single.observation()[key], got)
    ref.close()
    gym = gym_wrapper.GymWrapper(single)
    space = gym.observation_space
    assert space['pair'].shape == (36, 36) and space['pair'].dtype == np.uint8 and space['layer'].shape == (25, 4)
    obs, reward, done, info = gym.step(np.array([0.1, -0.2]))
    assert obs['odd'].shape == (7, 11) and obs['odd'].dtype == np.uint8
    single.close()


def test_fitted_layers_move_the_rows():
    import torch
    obs = {'p': observers.Contacts(('prey', 'shapes', 'walls', 'agent')), 'l': observers.Contacts('agent', ('prey', 'walls'), mode='layer')}
    env = _env('ray_zoo', 8, obs, seed=6, layer_capacity={'prey': 20})
    ts = env.reset()
    torch.manual_seed(2)
    for t in range(6):
        ts = env.step(env.random_action())
    check_contacts(env, ts.observation, 'before')
    rows_before = env.contact_rows('p')[0]
    caps = env.fit_layer_capacity()
    assert caps and caps['prey'] < 20
    got = env._observation()
    rows = env.contact_rows('p')[0]
    assert len(rows) == len(rows_before) - (20 - caps['prey']) and rows.index(('shapes', 0)) == caps['prey']
    assert got['p'] is env.tables['p'] and tuple(got['p'].shape) == (8, len(rows), len(rows))
    assert env.observation_spec()['p'].shape == (len(rows), len(rows))
    check_contacts(env, got, 'fitted')
    for t in range(3):
        ts = env.step(env.random_action())
        check_contacts(env, ts.observation, 'after %d' % t)
    env.close()


def test_engine_refuses_bad_contacts():
    env = _env('ray_zoo', 2, {'c%d' % k: observers.Contacts('agent', 'walls') for k in range(_abi.MOOG_MAX_CONTACTS)})
    lib, idx = env._lib, ctypes.c_int32()
    good = dict(env.compiled.contacts)['c0']
    assert lib.moog_engine_add_contacts(env._handle, ctypes.byref(good), ctypes.byref(idx)) == _abi.MOOG_E_INVALID   # a fifth
    assert b'MOOG_MAX_CONTACTS' in lib.moog_last_error()
    env.close()
    env = _env('ray_zoo', 2, {})
    S = env.layout.S
    for edit, word in ((lambda T: setattr(T, 'n_rows_0', 0), b'n_rows_0 outside 1 .. MOOG_MAX_SLOTS'),
                       (lambda T: setattr(T, 'n_rows_1', 0), b'n_rows_1 outside 1 .. MOOG_MAX_SLOTS'),
                       (lambda T: setattr(T, 'n_rows_0', 257), b'n_rows_0 outside'), (lambda T: setattr(T, 'n_rows_1', 257), b'n_rows_1 outside'),
                       (lambda T: setattr(T, 'mode', 7), b'mode is neither'), (lambda T: setattr(T, 'flags', 6), b'unknown flag bits'),
                       (lambda T: T.row_slot_0.__setitem__(0, S), b'outside the layout'), (lambda T: T.row_slot_1.__setitem__(0, -1), b'outside the layout'),
                       (lambda T: T.row_slot_1.__setitem__(1, T.row_slot_1[0]), b'two rows of one list')):
        T = _abi.Contacts.from_buffer_copy(good)
        edit(T)
        assert lib.moog_engine_add_contacts(env._handle, ctypes.byref(T), ctypes.byref(idx)) == _abi.MOOG_E_INVALID
        assert word in lib.moog_last_error(), (word, lib.moog_last_error())
    assert lib.moog_engine_set_contacts_buffer(env._handle, 0, None) == _abi.MOOG_E_INVALID   # (none was added)
    assert b'no such contacts observer' in lib.moog_last_error()
    _engine.check(lib, lib.moog_engine_observe_contacts(env._handle, env._stream()))           # nothing bound: nothing to do
    env.reset()
    env.close()


def test_one_bracket_per_call():
    """A table, two sensors and a contacts observer on one handle: MOOG_K_TABLES counts one per reset / step call."""
    import torch
    env = _env('ray_zoo', 4, {'touch': observers.Contacts(('agent', 'shapes'), ('walls', 'shapes', 'prey'))}, seed=1)
    assert len(env.compiled.tables) == 1 and len(env.compiled.sensors) == 2 and len(env.compiled.contacts) == 1
    env.set_timing(True, kernels=[_abi.MOOG_K_TABLES])
    env.reset()
    torch.manual_seed(1)
    for t in range(8):
        env.step(env.random_action())
    assert env.kernel_time(_abi.MOOG_K_TABLES)[1] == 9
    env.close()


def test_nothing_else_moved():
    """colliding_predators_32 at 32 envs with a contacts observer beside the PILRenderer and without: after 8 calls the time
    steps, the frames and both records are bit-equal, and both engines step and draw with the same kernels."""
    import torch
    names = tuple(host.layers_with_slots('colliding_predators_32'))
    plain = _env('colliding_predators_32', 32, {}, seed=9)
    cont = _env('colliding_predators_32', 32, {'c': observers.Contacts(names)}, seed=9)
    assert bytes(plain.compiled.program) == bytes(cont.compiled.program)
    assert plain.step_kernel() == cont.step_kernel() and plain.raster_path() == cont.raster_path()
    assert plain.kernel_variant == cont.kernel_variant
    a, b = plain.reset(), cont.reset()
    rs = np.random.RandomState(2)
    for t in range(8):
        act = rs.uniform(-1, 1, size=(32, 2))
        a, b = plain.step(act), cont.step(act)
        torch.cuda.synchronize()
        for x, y in ((a.step_type, b.step_type), (a.reward, b.reward), (a.discount, b.discount),
                     (a.observation['image'], b.observation['image']), (plain.state_i32, cont.state_i32)):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True), t
        assert np.array_equal(plain.state_f64.cpu().numpy().view(np.uint64), cont.state_f64.cpu().numpy().view(np.uint64)), t
    check_contacts(cont, b.observation, 'last')
    assert plain.step_kernel() == cont.step_kernel() and plain.raster_path() == cont.raster_path()
    assert list(a.observation) == ['image'] and list(b.observation) == ['image', 'c']
    plain.close()
    cont.close()
