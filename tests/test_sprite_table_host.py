"""SpriteTable observer without a GPU: the host model of the sprite-table kernel (csrc/moog_sprite_table.h compiled with
g++, tests/csrc/sprite_table_model.cpp: the conversions, the descriptors and the lane function the kernel runs, its grid
walked lane by lane) against the reference's recordings and against numpy's casts, the lowering, and the library's symbols.
Every comparison is bit for bit: the expected value is numpy's cast of a number both sides hold exactly.  The kernel
itself is held to the same expectations by tests/test_sprite_table_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers
from moog import _abi
from moog import _compiler
from moog import _engine
from moog import observers
from moog.observers import sprite_table
from moog_demos import example_configs

SRC = os.path.join(helpers.REPO, 'tests', 'csrc', 'sprite_table_model.cpp')
ALL = observers.SpriteTable.ALL_COLUMNS
DEFAULT = observers.SpriteTable.DEFAULT_COLUMNS
# recordings the model packs: the three the tool measures and one whose rules append to layers (rules_zoo level 1:
# CreateSprites into `prey` and `predators`, VanishOnContact, a timed purge)
RECORDINGS = ('pong', 'colliding_predators_32', 'chase_avoid_torus', 'rules_zoo_l1')


def build_model():
    return helpers.build_host_model(SRC, 'sprite_table_model')


@pytest.fixture(scope='module')
def model():
    return build_model()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def same_bits(got, want):
    """Bit for bit; a NaN compares as a NaN (its payload is not numpy's to define)."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return bool(np.all((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))


def model_pack(m, P, tables, f64, i32, chunk_envs=0, odd_start=False):
    """One model launch over host records: [table tensor, ...].  odd_start: float16 buffers start in the middle of a dword."""
    n = f64.shape[0]
    arr = (_abi.Table * len(tables))(*tables)
    keep, outs = [], []
    for T in tables:
        dt = sprite_table.table_dtype(T)
        count = n * T.n_rows * T.n_cols
        raw = np.full(count + 4, 0x5555, np.uint16) if dt == np.float16 else np.full(count + 1, 0x55555555, np.uint32)
        off = 1 if (odd_start and dt == np.float16) else 0
        assert raw.ctypes.data % 4 == 0
        keep.append(raw)
        outs.append((raw, off, count, dt, T))
    ptrs = (ctypes.c_void_p * len(tables))(*[raw.ctypes.data + off * raw.itemsize for raw, off, _, _, _ in outs])
    err = ctypes.create_string_buffer(256)
    f64, i32 = np.ascontiguousarray(f64, np.float64), np.ascontiguousarray(i32, np.int32)
    rc = m.st_model_pack(ctypes.byref(P), arr, len(tables), f64.ctypes.data_as(ctypes.c_void_p),
                         i32.ctypes.data_as(ctypes.c_void_p), n, ptrs, int(chunk_envs), err, 256)
    if rc != 0:
        raise ValueError(err.value.decode())
    res = []
    for raw, off, count, dt, T in outs:
        # nothing outside the table is touched
        assert np.all(raw[:off] == raw.dtype.type(0x5555 if dt == np.float16 else 0x55555555))
        assert np.all(raw[off + count:] == raw.dtype.type(0x5555 if dt == np.float16 else 0x55555555))
        res.append(raw[off:off + count].view(dt).reshape(n, T.n_rows, T.n_cols).copy())
    return res


def fixture_records(name, c):
    """(fx, f64 [T, ...], i32 [T, ...]): the records of every recorded call, one env per call."""
    fx = helpers.fixture(name, 0)
    n = len(fx['step_type'])
    f64 = np.zeros((n, c.layout.f64_per_env))
    i32 = np.zeros((n, c.layout.i32_per_env), np.int32)
    for t in range(n):
        helpers.records_from_fixture(fx, t, c, f64, i32, env=t)
    return fx, f64, i32


def expected_from_fixture(fx, c, T, columns, rows_slots):
    """The table of every recorded call from the recording's own attributes, cast by numpy; dead rows zero."""
    P = c.program
    src = {
        'x': fx['pos'][:, :, 0], 'y': fx['pos'][:, :, 1], 'x_vel': fx['vel'][:, :, 0], 'y_vel': fx['vel'][:, :, 1],
        'angle': fx['angle'], 'angle_vel': fx['angvel'], 'mass': fx['mass'], 'c0': fx['color'][:, :, 0],
        'c1': fx['color'][:, :, 1], 'c2': fx['color'][:, :, 2], 'opacity': fx['opacity'], 'scale': fx['scale'],
        'aspect_ratio': fx['aspect'], 'alive': fx['alive'], 'n_vertices': fx['nverts'],
        'layer': np.broadcast_to(np.array([P.slot_layer[s] for s in range(c.layout.S)]), fx['alive'].shape),
        'shape_id': np.zeros(fx['alive'].shape, np.int32),   # (the recordings hold no shape id; records_from_fixture leaves 0)
    }
    dt = sprite_table.table_dtype(T)
    alive = fx['alive'][:, rows_slots] != 0
    out = np.zeros((alive.shape[0], len(rows_slots), len(columns)), dt)
    with np.errstate(all='ignore'):
        for k, col in enumerate(columns):
            out[:, :, k] = np.where(alive, np.asarray(src[col])[:, rows_slots].astype(dt), dt.type(0))
    return out


def compile_with(name, tables, keep=False):
    cfg = example_configs.load(name)
    obs = dict(cfg['observers'])
    obs.update(tables)
    cfg['observers'] = obs
    return _compiler.compile_config(layer_capacity=example_configs.capacity(name), keep_sprite_factors=keep, **cfg)


@pytest.mark.parametrize('name', RECORDINGS)
def test_model_against_the_recordings(model, name):
    """Every recorded call of the recording, default columns and all columns, float32 and float16, in one model launch of four
    tables: equal to the recording's attributes cast by numpy."""
    tables = {'d32': observers.SpriteTable(), 'd16': observers.SpriteTable(dtype='float16'),
              'a32': observers.SpriteTable(columns=ALL), 'a16': observers.SpriteTable(columns=ALL, dtype='float16')}
    c = compile_with(name, tables, keep=True)
    fx, f64, i32 = fixture_records(name, c)
    keys = [k for k, _ in c.tables]
    assert keys == list(tables)
    got = model_pack(model, c.program, [T for _, T in c.tables], f64, i32)
    for (key, T), g in zip(c.tables, got):
        slots = [T.row_slot[r] for r in range(T.n_rows)]
        assert slots == list(range(c.layout.S))
        want = expected_from_fixture(fx, c, T, tables[key].columns, slots)
        assert same_bits(g, want), (name, key, np.argwhere(bits(g) != bits(want))[:5])
        assert np.all(g[fx['alive'] == 0] == 0)
    # the same records under a program without sprite_factors (the default columns need none): same default tables
    c0 = compile_with(name, {'d32': tables['d32'], 'd16': tables['d16']})
    fx, f64, i32 = fixture_records(name, c0)
    got0 = model_pack(model, c0.program, [T for _, T in c0.tables], f64, i32)
    assert same_bits(got0[0], got[0]) and same_bits(got0[1], got[1])


def test_model_appended_layer_rows_are_the_reference_list(model):
    """rules_zoo level 1: row i of a layer that rules append to is the reference's state[layer][i] -- after sprites were
    created (call 16: three prey, two predators) and after some vanished (call 17: the predators purged)."""
    tables = {'t': observers.SpriteTable(layers=('predators', 'prey'), columns=('alive', 'x', 'y'))}
    c = compile_with('rules_zoo_l1', tables)
    fx, f64, i32 = fixture_records('rules_zoo_l1', c)
    (key, T), = c.tables
    g, = model_pack(model, c.program, [T], f64, i32)
    s_pred, n_pred = c.layer_slots['predators']
    s_prey, n_prey = c.layer_slots['prey']
    assert c.table_rows['t'] == [('predators', k) for k in range(n_pred)] + [('prey', k) for k in range(n_prey)]
    for t, n_live_pred, n_live_prey in ((16, 2, 3), (17, 0, 4)):
        assert int(fx['alive'][t, s_pred:s_pred + n_pred].sum()) == n_live_pred
        assert int(fx['alive'][t, s_prey:s_prey + n_prey].sum()) == n_live_prey
        for base, s0, n_live in ((0, s_pred, n_live_pred), (n_pred, s_prey, n_live_prey)):
            for i in range(n_live):   # packed at the front, in list order
                assert g[t, base + i, 0] == 1
                assert g[t, base + i, 1] == np.float32(fx['pos'][t, s0 + i, 0]) and g[t, base + i, 2] == np.float32(fx['pos'][t, s0 + i, 1])
            assert np.all(g[t, base + n_live:base + (n_pred if base == 0 else n_prey)] == 0)


def test_model_grid_edges(model):
    """What the launch's grid must cover: element counts that are no multiple of the workgroup, an odd float16 count, a
    float16 buffer that starts in the middle of a dword (a sub-batch's slice), tables of different sizes in one launch, and
    envs in several chunks."""
    tables = {'a': observers.SpriteTable(layers=('agent',), columns=('x', 'mass', 'alive'), dtype='float16'),   # 1 row x 3
              'b': observers.SpriteTable(columns=ALL),
              'c': observers.SpriteTable(layers=('predators', 'walls'), columns=('y', 'x', 'layer', 'n_vertices', 'c2'), dtype='float16'),
              'd': observers.SpriteTable(layers=('prey',), columns=('opacity',))}
    c = compile_with('rules_zoo_l1', tables, keep=True)
    fx, f64, i32 = fixture_records('rules_zoo_l1', c)
    T = [t for _, t in c.tables]
    assert (T[0].n_rows * T[0].n_cols) % 2 == 1 and (T[2].n_rows * T[2].n_cols) % 2 == 0
    ref = model_pack(model, c.program, T, f64, i32)
    for k, (key, t) in enumerate(c.tables):
        slots = [t.row_slot[r] for r in range(t.n_rows)]
        assert same_bits(ref[k], expected_from_fixture(fx, c, t, tables[key].columns, slots)), key
    for n in (1, 3, 67, 81):   # (81 x 3 is odd; 3 x 3 and 67 x 3 too)
        for chunk, odd in ((0, False), (0, True), (1, True), (2, False), (7, True), (64, False)):
            got = model_pack(model, c.program, T, f64[:n], i32[:n], chunk_envs=chunk, odd_start=odd)
            for k in range(len(T)):
                assert same_bits(got[k], ref[k][:n]), (n, chunk, odd, k)
    # one table alone gives what it gives beside the others
    for k in range(len(T)):
        assert same_bits(model_pack(model, c.program, [T[k]], f64, i32, odd_start=True)[0], ref[k])


def test_model_refuses_what_the_engine_refuses(model):
    """moog_st_describe is the engine's check (moog_engine_add_table): a slot outside the layout, scale without o_scale, an
    unknown column, sizes out of range."""
    c = compile_with('pong', {'t': observers.SpriteTable()})
    f64, i32 = np.zeros((1, c.layout.f64_per_env)), np.zeros((1, c.layout.i32_per_env), np.int32)
    (_, good), = c.tables

    def variant(**kw):
        T = _abi.Table.from_buffer_copy(good)
        for k, v in kw.items():
            if k == 'slot0':
                T.row_slot[0] = v
            elif k == 'col0':
                T.cols[0] = v
            else:
                setattr(T, k, v)
        return T
    model_pack(model, c.program, [variant()], f64, i32)
    for kw, word in ((dict(slot0=c.layout.S), 'slot'), (dict(slot0=-1), 'slot'), (dict(col0=_abi.MOOG_TCOL_SCALE), 'o_scale'),
                     (dict(col0=_abi.MOOG_TCOL_ASPECT), 'o_aspect'), (dict(col0=_abi.MOOG_TCOL_COUNT), 'column'),
                     (dict(col0=-1), 'column'), (dict(n_rows=0), 'n_rows'), (dict(n_rows=_abi.MOOG_MAX_SLOTS + 1), 'n_rows'),
                     (dict(n_cols=0), 'n_cols'), (dict(n_cols=_abi.MOOG_MAX_TABLE_COLS + 1), 'n_cols'), (dict(dtype=2), 'dtype')):
        with pytest.raises(ValueError, match=word):
            model_pack(model, c.program, [variant(**kw)], f64, i32)


# ---- conversions ---------------------------------------------------------------------------------------------------------
def convert(m, x):
    x = np.ascontiguousarray(x, np.float64)
    f32, f16 = np.zeros(x.shape, np.uint32), np.zeros(x.shape, np.uint16)
    m.st_model_convert(x.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(x.size), f32.ctypes.data_as(ctypes.c_void_p),
                       f16.ctypes.data_as(ctypes.c_void_p))
    return f32.view(np.float32), f16.view(np.float16)


def check_conversions(m, x):
    f32, f16 = convert(m, x)
    with np.errstate(all='ignore'):
        w32, w16 = x.astype(np.float32), x.astype(np.float16)
    bad32 = ~((bits(f32) == bits(w32)) | (np.isnan(f32) & np.isnan(w32)))
    bad16 = ~((bits(f16) == bits(w16)) | (np.isnan(f16) & np.isnan(w16)))
    assert not bad32.any(), [(v.hex(), a, b) for v, a, b in zip(x[bad32][:5], f32[bad32], w32[bad32])]
    assert not bad16.any(), [(v.hex(), a, b) for v, a, b in zip(x[bad16][:5], f16[bad16], w16[bad16])]


def test_conversions_random_bit_patterns(model):
    rs = np.random.RandomState(7)
    x = np.frombuffer(rs.bytes(8 * 1000000), np.uint64).view(np.float64)
    check_conversions(model, x)
    # the same count again inside the exponent range where float16 and float32 are not all zero / inf
    e = rs.randint(1023 - 160, 1023 + 130, size=1000000).astype(np.uint64)
    b = (np.frombuffer(rs.bytes(8 * 1000000), np.uint64) & np.uint64(0x800fffffffffffff)) | (e << np.uint64(52))
    check_conversions(model, b.view(np.float64))


def test_conversions_around_every_float16_tie(model):
    """The double-rounding set: every float16 tie (the midpoint of two neighbouring float16 values, subnormals and the
    overflow tie 65520 included), both signs, moved by 0 and by +- 1 float64 ulp and +- 1, 1/2, 1/4 and 1/128 float32 ulp."""
    h = np.arange(0, 0x7c00, dtype=np.uint16)
    lo = h.view(np.float16).astype(np.float64)
    hi = np.append(lo[1:], 65536.0)
    tie = (lo + hi) / 2
    assert tie[-1] == 65520.0 and np.all(tie > lo) and np.all(tie < hi)
    ulp32 = np.spacing(tie.astype(np.float32)).astype(np.float64)
    xs = [tie, np.nextafter(tie, np.inf), np.nextafter(tie, -np.inf)]
    for f in (1.0, 0.5, 0.25, 1.0 / 128):
        xs += [tie + f * ulp32, tie - f * ulp32]
    x = np.concatenate(xs)
    x = np.concatenate([x, -x])
    named = 1 + 2.0 ** -11 + 2.0 ** -30
    assert named in x   # the tie 1 + 2^-11 moved up by 1/128 of float32's ulp there
    check_conversions(model, x)
    f32, f16 = convert(model, np.array([named]))
    assert float(f16[0]) == 1 + 2.0 ** -10   # (a float32 intermediate would give 1.0)
    # and the float32 ties, for the float32 conversion: midpoints of neighbouring float32 values around a spread of exponents
    rs = np.random.RandomState(11)
    a = np.frombuffer(rs.bytes(4 * 200000), np.uint32) & np.uint32(0x7f7fffff)
    a = a[a < 0x7f7fffff]
    t32 = (a.view(np.float32).astype(np.float64) + (a + np.uint32(1)).view(np.float32).astype(np.float64)) / 2
    y = np.concatenate([t32, np.nextafter(t32, np.inf), np.nextafter(t32, -np.inf)])
    check_conversions(model, np.concatenate([y, -y]))


def test_conversions_special_values(model):
    tiny16, tiny32 = 2.0 ** -24, 2.0 ** -149
    x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 65519.999, 65520.0, np.nextafter(65520.0, 0), 65504.0, 65536.0,
                  1e300, -1e300, 5e-324, -5e-324, 2.2250738585072014e-308,
                  tiny16, tiny16 / 2, np.nextafter(tiny16 / 2, 1), np.nextafter(tiny16 / 2, 0), 1.5 * tiny16, 2.5 * tiny16,
                  2.0 ** -14, np.nextafter(2.0 ** -14, 0), 2.0 ** -14 - 2.0 ** -25, 1023 * tiny16, 1023.5 * tiny16,
                  tiny32, tiny32 / 2, np.nextafter(tiny32 / 2, 1), np.nextafter(tiny32 / 2, 0), 1.5 * tiny32, 2.5 * tiny32,
                  2.0 ** -126, np.nextafter(2.0 ** -126, 0), 2.0 ** -126 - 2.0 ** -150,
                  3.4028234663852886e38, 3.4028235677973366e38, np.nextafter(3.4028235677973366e38, 0), 3.5e38,
                  1.0, -1.0, 255.0, 0.1, 1 / 3.0, 2.0 ** 31, -2.0 ** 31])
    check_conversions(model, x)
    check_conversions(model, np.concatenate([x, -x]))
    # every float16 subnormal and every int32-sized integer edge the int columns can hold
    check_conversions(model, np.arange(0, 1025) * tiny16)
    check_conversions(model, np.array([-2 ** 31, 2 ** 31 - 1, 2047, 2048, 2049, 4097, 65519, 65520, 16777217, 16777219], np.float64))
    f32, f16 = convert(model, np.array([np.nan, 65519.999, 65520.0]))
    assert np.isnan(f32[0]) and np.isnan(f16[0]) and f16[1] == np.float16(65504) and np.isinf(f16[2])


# ---- lowering ------------------------------------------------------------------------------------------------------------
def program_bytes(c):
    return bytes(c.program)


def program_hash(c):
    lib = _engine.load_library()
    h = ctypes.c_uint64()
    _engine.check(lib, lib.moog_program_step_kernel(ctypes.byref(c.program), None, None, ctypes.byref(h)))
    return h.value


@pytest.mark.parametrize('name', ('pong', 'colliding_predators_32', 'rules_zoo_l1'))
def test_tables_leave_the_program_alone(name):
    plain = helpers.compiled(name)
    c = compile_with(name, {'t': observers.SpriteTable(), 'h': observers.SpriteTable(dtype='float16', columns=('alive', 'layer'))})
    assert program_bytes(c) == program_bytes(plain) and program_hash(c) == program_hash(plain)
    assert [k for k, _ in c.tables] == ['t', 'h'] and plain.tables == [] and plain.table_rows == {}
    assert c.observer_key == plain.observer_key and len(c.views) == len(plain.views)


def test_a_config_of_tables_alone_draws_no_frames():
    cfg = example_configs.load('pong')
    cfg['observers'] = {'table': observers.SpriteTable(), 'state': observers.RawState()}
    c = _compiler.compile_config(**cfg)
    assert c.observer_key is None and c.views == [] and (c.program.render.width, c.program.render.height) == (0, 0)
    cfg['observers'] = {'state': observers.RawState()}
    assert program_bytes(_compiler.compile_config(**cfg)) == program_bytes(c)


def test_layers_columns_and_rows():
    c = compile_with('rules_zoo_l1', {
        'all': observers.SpriteTable(),
        'some': observers.SpriteTable(layers=('predators', 'agent'), columns=('mass', 'alive', 'shape_id'), dtype='float16')})
    P = c.program
    names = list(c.layer_names)
    assert names == ['walls', 'prey', 'agent', 'predators']
    T_all, T_some = c.tables[0][1], c.tables[1][1]
    assert T_all.n_rows == c.layout.S and [T_all.row_slot[r] for r in range(T_all.n_rows)] == list(range(c.layout.S))
    assert c.table_rows['all'] == [(n, k) for li, n in enumerate(names) for k in range(P.layer_nslots[li])]
    assert [T_all.cols[k] for k in range(T_all.n_cols)] == [sprite_table.COLUMN_IDS[x] for x in DEFAULT]
    assert T_all.dtype == _abi.MOOG_TABLE_F32 and T_some.dtype == _abi.MOOG_TABLE_F16
    s_pred, n_pred = c.layer_slots['predators']
    s_agent, n_agent = c.layer_slots['agent']
    assert (n_pred, n_agent) == (8, 1)   # (the recipe's LAYER_CAPACITY: rows follow capacity, not what is alive)
    assert [T_some.row_slot[r] for r in range(T_some.n_rows)] == list(range(s_pred, s_pred + 8)) + [s_agent]
    assert c.table_rows['some'] == [('predators', k) for k in range(8)] + [('agent', 0)]
    assert [T_some.cols[k] for k in range(3)] == [_abi.MOOG_TCOL_MASS, _abi.MOOG_TCOL_ALIVE, _abi.MOOG_TCOL_SHAPE_ID]
    # other capacities, other row counts
    cfg = example_configs.load('rules_zoo_l1')
    cfg['observers'] = dict(cfg['observers'], some=observers.SpriteTable(layers=('predators',)))
    c2 = _compiler.compile_config(layer_capacity={'prey': 8, 'predators': 5}, **cfg)
    assert c2.tables[0][1].n_rows == 5


def test_observation_spec():
    t32 = observers.SpriteTable()
    t16 = observers.SpriteTable(layers=('agent', 'walls'), columns=('x', 'y', 'alive'), dtype='float16')
    with pytest.raises(ValueError, match='build the environment'):
        t32.observation_spec()
    c = compile_with('rules_zoo_l1', {'t32': t32, 't16': t16})
    s32, s16 = t32.observation_spec(), t16.observation_spec()
    assert s32.shape == (c.layout.S, 12) and s32.dtype == np.float32
    assert s16.shape == (5, 3) and s16.dtype == np.float16
    assert sprite_table.table_spec(c.tables[1][1]).shape == (5, 3)
    assert (t32.dtype, t16.dtype, t16.layers, t16.columns) == (np.float32, np.float16, ('agent', 'walls'), ('x', 'y', 'alive'))
    assert observers.SpriteTable.DEFAULT_COLUMNS == ('alive', 'x', 'y', 'x_vel', 'y_vel', 'angle', 'angle_vel', 'c0', 'c1', 'c2',
                                                     'opacity', 'mass')
    assert set(ALL) == set(sprite_table.COLUMN_IDS) and len(ALL) == _abi.MOOG_TCOL_COUNT == _abi.MOOG_MAX_TABLE_COLS


def test_what_is_refused():
    for kw in (dict(columns=('x', 'shape')), dict(columns=('metadata',)), dict(columns=()), dict(columns=('x', 'x')),
               dict(dtype='float64'), dict(dtype='int32'), dict(columns='x'),
               dict(layers='walls'), dict(layers=('walls', 'walls'))):
        with pytest.raises(ValueError):
            observers.SpriteTable(**kw)
    with pytest.raises(ValueError, match='unknown layer'):
        compile_with('pong', {'t': observers.SpriteTable(layers=('nowhere',))})
    for col in ('scale', 'aspect_ratio'):
        with pytest.raises(ValueError, match='keep_sprite_factors=True'):
            compile_with('pong', {'t': observers.SpriteTable(columns=('x', col))})
        c = compile_with('pong', {'t': observers.SpriteTable(columns=('x', col))}, keep=True)
        assert c.program.sprite_factors == 1
    assert helpers.compiled('pong').program.sprite_factors == 0   # (and a table never switches it on)
    four = {'t%d' % k: observers.SpriteTable() for k in range(_abi.MOOG_MAX_TABLES)}
    assert len(compile_with('pong', four).tables) == _abi.MOOG_MAX_TABLES == 4
    with pytest.raises(NotImplementedError, match='MOOG_MAX_TABLES'):
        compile_with('pong', dict(four, fifth=observers.SpriteTable()))

    class Other(observers.AbstractObserver):
        pass
    with pytest.raises(NotImplementedError, match='Other'):
        compile_with('pong', {'o': Other()})


def test_library_symbols():
    lib = _engine.load_library()
    for sym in ('moog_engine_add_table', 'moog_engine_set_table_buffer', 'moog_engine_observe_tables'):
        assert sym in _engine.SYMBOLS and hasattr(lib, sym), sym
    assert lib.moog_abi_version() == 31 == _abi.MOOG_ABI_VERSION and _abi.MOOG_PROGRAM_VERSION == 30
    assert (_abi.MOOG_K_TABLES, _abi.MOOG_K_COUNT) == (4, 5)
    # (null handles are refused, not dereferenced)
    idx = ctypes.c_int32()
    assert lib.moog_engine_add_table(None, ctypes.byref(_abi.Table()), ctypes.byref(idx)) == _abi.MOOG_E_INVALID
    assert lib.moog_engine_set_table_buffer(None, 0, None) == _abi.MOOG_E_INVALID
    assert lib.moog_engine_observe_tables(None, None) == _abi.MOOG_E_INVALID
    assert lib.moog_last_error()
