"""RaySensor observer without a GPU: the host model of the ray-sensor kernel (csrc/moog_ray_sensor.h compiled with g++
-O2 -ffp-contract=off, tests/csrc/ray_sensor_model.cpp: the descriptors and the wave function the kernel runs, walked lane by
lane) against known answers on planted records and against an independent numpy implementation over the reference's
recordings, bit for bit; the edge-chunk boundary; the lowering and the refusals; and the share of rays that a rotation by the
origin's angle leaves undecided.  The kernel itself is held to the same expectations by tests/test_ray_sensor_gpu.py."""
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
from moog_demos import example_configs

SRC = os.path.join(helpers.REPO, 'tests', 'csrc', 'ray_sensor_model.cpp')
RECORDINGS = ('pong', 'colliding_predators_32', 'rules_zoo_l1', 'falling_balls_64')
F32, F16 = _abi.MOOG_TABLE_F32, _abi.MOOG_TABLE_F16


def build_model():
    return helpers.build_host_model(SRC, 'ray_sensor_model')


@pytest.fixture(scope='module')
def model():
    return build_model()


def sensor_dtype(T):
    return np.dtype(np.float16 if T.dtype == F16 else np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return bool(np.all(bits(got) == bits(want)))


def model_cast(m, P, sensors, f64, i32, chunk=0, cs=None):
    """One model launch over host records: [[n, rays, 2] readings per sensor].  cs: [sensors, n, 2] cos / sin to rotate by."""
    n = f64.shape[0]
    arr = (_abi.Sensor * len(sensors))(*sensors)
    outs = []
    for T in sensors:
        dt = sensor_dtype(T)
        count = n * T.n_rays * 2
        raw = np.full(count + 4, 0x5555, np.uint16) if dt == np.float16 else np.full(count + 2, 0x55555555, np.uint32)
        assert raw.ctypes.data % 4 == 0
        outs.append((raw, count, dt, T))
    ptrs = (ctypes.c_void_p * len(sensors))(*[raw.ctypes.data for raw, _, _, _ in outs])
    err = ctypes.create_string_buffer(256)
    f64, i32 = np.ascontiguousarray(f64, np.float64), np.ascontiguousarray(i32, np.int32)
    if cs is not None:
        cs = np.ascontiguousarray(cs, np.float64)
        assert cs.shape == (len(sensors), n, 2)
    rc = m.rs_model_cast(ctypes.byref(P), arr, len(sensors), f64.ctypes.data_as(ctypes.c_void_p),
                         i32.ctypes.data_as(ctypes.c_void_p), n, ptrs, int(chunk),
                         None if cs is None else cs.ctypes.data_as(ctypes.c_void_p), err, 256)
    if rc != 0:
        raise ValueError(err.value.decode())
    res = []
    for raw, count, dt, T in outs:
        assert np.all(raw[count:] == raw.dtype.type(0x5555 if dt == np.float16 else 0x55555555))   # nothing beyond the tensor
        res.append(raw[:count].view(dt).reshape(n, T.n_rays, 2).copy())
    return res


# ---- the independent implementation ----------------------------------------------------------------------------------
def numpy_cast(c, T, f64, i32, cs=None):
    """What the header's documentation says, as plain float64 numpy: per env every ray against every edge of every target,
    then the nearest kept hit per ray (ties: the lowest row).  cs: [n, 2] cos / sin of the origin's angle (default numpy's)."""
    P, L = c.program, c.layout
    n = f64.shape[0]
    dt = sensor_dtype(T)
    out = np.zeros((n, T.n_rays, 2), dt)
    d = np.array([[T.dirs[k][0], T.dirs[k][1]] for k in range(T.n_rays)], np.float64)
    slots = [T.row_slot[r] for r in range(T.n_rows)]
    ids, last_layer, layer_id = [], None, 0
    for r, s in enumerate(slots):
        if T.mode == _abi.MOOG_SENSOR_INSTANCE:
            ids.append(r + 1)
        else:
            if P.slot_layer[s] != last_layer:
                layer_id, last_layer = layer_id + 1, P.slot_layer[s]
            ids.append(layer_id)
    origin = T.origin_slot
    with np.errstate(all='ignore'):
        for e in range(n):
            f, q = f64[e], i32[e]
            out[e, :, 0] = np.float64(T.max_range).astype(dt)
            if not q[L.o_flags + origin] & _abi.MOOG_F_ALIVE:
                continue
            O = f[L.o_pos + 2 * origin:L.o_pos + 2 * origin + 2]
            D = d
            if T.flags & _abi.MOOG_SENSOR_FOLLOW_ANGLE:
                co, si = (np.cos(f[L.o_angle + origin]), np.sin(f[L.o_angle + origin])) if cs is None else cs[e]
                D = np.stack([co * d[:, 0] - si * d[:, 1], si * d[:, 0] + co * d[:, 1]], axis=1)
            A, B, row = [], [], []
            for r, s in enumerate(slots):
                if s == origin or not q[L.o_flags + s] & _abi.MOOG_F_ALIVE:
                    continue
                if (T.flags & _abi.MOOG_SENSOR_VISIBLE_ONLY) and not q[L.o_opacity + s] > 0:
                    continue
                nv = int(q[L.o_nverts + s])
                if nv < 2:
                    continue
                o = L.o_verts + 2 * P.slot_voff[s]
                V = f[o:o + 2 * nv].reshape(nv, 2)
                A.append(V)
                B.append(np.roll(V, -1, axis=0))
                row += [r] * nv
            if not A:
                continue
            A, B, row = np.concatenate(A), np.concatenate(B), np.array(row)
            E, W = B - A, A - O
            Dx, Dy = D[:, 0:1], D[:, 1:2]
            Ex, Ey, Wx, Wy = E[None, :, 0], E[None, :, 1], W[None, :, 0], W[None, :, 1]
            den = Dx * Ey - Dy * Ex
            nt = np.broadcast_to(Wx * Ey - Wy * Ex, den.shape)
            nu = Wx * Dy - Wy * Dx
            sg = np.sign(den)
            ok = np.isfinite(den) & (den != 0) & (sg * nt >= 0) & (sg * nu >= 0) & (sg * nu <= sg * den)
            t = nt / den
            ok &= t <= T.max_range
            for k in range(T.n_rays):
                idx = np.nonzero(ok[k])[0]
                if len(idx) == 0:
                    continue
                best = t[k, idx].min()
                r = row[idx[t[k, idx] == best]].min()
                out[e, k, 0] = np.float64(best + 0.0).astype(dt)
                out[e, k, 1] = dt.type(ids[r])
    return out


# ---- configs and records ---------------------------------------------------------------------------------------------
def compile_with(name, extra, alone=False):
    cfg = example_configs.load(name)
    obs = {} if alone else {k: o for k, o in cfg['observers'].items() if not isinstance(o, observers.RaySensor)}
    obs.update(extra)
    cfg['observers'] = obs
    return _compiler.compile_config(layer_capacity=example_configs.capacity(name), **cfg)


def fixture_records(name, c):
    """(fx, f64 [T, ...], i32 [T, ...]): the records of every recorded call, one env per call (as
    test_sprite_table_host.fixture_records)."""
    fx = helpers.fixture(name, 0)
    n = len(fx['step_type'])
    f64 = np.zeros((n, c.layout.f64_per_env))
    i32 = np.zeros((n, c.layout.i32_per_env), np.int32)
    for t in range(n):
        helpers.records_from_fixture(fx, t, c, f64, i32, env=t)
    return fx, f64, i32


def origin_layer_of(name):
    names = list(helpers.compiled(name).layer_names)
    slots = helpers.compiled(name).layer_slots
    return [k for k in names if slots[k][1] > 0][-1]   # ('agent' wherever it holds a sprite; falling_balls: 'balls')


def recording_sensors(name):
    o = origin_layer_of(name)
    return {'i32': observers.RaySensor(o, num_rays=32, max_range=2.0),
            'i16': observers.RaySensor(o, num_rays=7, max_range=0.4, dtype='float16', heading=0.3),
            'l32': observers.RaySensor(o, num_rays=65, max_range=0.6, mode='layer', visible_only=False),
            'l16': observers.RaySensor(o, num_rays=256, fov=np.pi, max_range=2.0, mode='layer', dtype='float16')}


def zoo_states(c, n=24, steps=6, seed=11):
    """ray_zoo records without a GPU: the CPU oracle's, after a reset and a few steps."""
    o = helpers.OracleEnv(c, n_envs=n, seed=seed)
    o.reset(render=False)
    rs = np.random.RandomState(seed)
    for _ in range(steps):
        o.step(rs.uniform(-1, 1, size=(n, 2)), render=False)
    return o.f64.copy(), o.i32.copy()


def cos_sin(c, sensors, f64, delta=0.0):
    """[sensors, n, 2]: numpy's cos / sin of every sensor's origin angle (+ delta)."""
    L = c.layout
    ang = np.stack([f64[:, L.o_angle + T.origin_slot] + delta for T in sensors])
    return np.stack([np.cos(ang), np.sin(ang)], axis=-1)


def excused_rays(m, c, sensors, f64, i32):
    """([n, rays] bool per sensor, model readings with numpy's cos / sin): a ray is excused when re-running the model with
    the origin's angle moved by +-1e-12 rad changes that ray's id."""
    base = model_cast(m, c.program, sensors, f64, i32, cs=cos_sin(c, sensors, f64))
    ex = [np.zeros(b.shape[:2], bool) for b in base]
    for delta in (-1e-12, 1e-12):
        moved = model_cast(m, c.program, sensors, f64, i32, cs=cos_sin(c, sensors, f64, delta))
        for k in range(len(sensors)):
            ex[k] |= bits(moved[k][:, :, 1]) != bits(base[k][:, :, 1])
    return ex, base


# ---- planted records -------------------------------------------------------------------------------------------------
PLANT_DIRS = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))
ORIGIN = (0.25, 0.5)


def planted_sensor(c, max_range=2.0, visible_only=True, dtype=F32, mode=_abi.MOOG_SENSOR_INSTANCE):
    """A sensor over every slot (row = slot, id = slot + 1 in instance mode) from the agent, rays along +x, +y, -x, -y."""
    T = _abi.Sensor()
    S = c.layout.S
    T.n_rows, T.n_rays, T.origin_slot = S, len(PLANT_DIRS), c.layer_slots['agent'][0]
    T.flags = _abi.MOOG_SENSOR_VISIBLE_ONLY if visible_only else 0
    T.mode, T.dtype, T.max_range = mode, dtype, max_range
    for s in range(S):
        T.row_slot[s] = s
    for k, (x, y) in enumerate(PLANT_DIRS):
        T.dirs[k][0], T.dirs[k][1] = x, y
    return T


def plant(c, sprites, origin_alive=True, origin_verts=None):
    """One record: sprites = {slot: (vertices, opacity)}, the agent at ORIGIN."""
    P, L = c.program, c.layout
    f, q = np.zeros(L.f64_per_env), np.zeros(L.i32_per_env, np.int32)
    a = c.layer_slots['agent'][0]
    all_ = dict(sprites)
    if origin_alive:
        all_[a] = (origin_verts if origin_verts is not None else [(0.2, 0.45), (0.3, 0.45), (0.25, 0.55)], 255)
    for s, (verts, opacity) in all_.items():
        verts = np.asarray(verts, np.float64).reshape(-1, 2)
        assert len(verts) <= P.slot_vcap[s], (s, len(verts), P.slot_vcap[s])
        q[L.o_flags + s] = _abi.MOOG_F_ALIVE
        q[L.o_nverts + s] = len(verts)
        q[L.o_opacity + s] = opacity
        o = L.o_verts + 2 * P.slot_voff[s]
        f[o:o + 2 * len(verts)] = verts.ravel()
        f[L.o_pos + 2 * s:L.o_pos + 2 * s + 2] = np.nanmean(verts, axis=0) if np.isfinite(verts).any() else 0.0
    f[L.o_pos + 2 * a:L.o_pos + 2 * a + 2] = ORIGIN
    return f, q


def box(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def planted_cases(c):
    """[(name, f64, i32, sensor arguments, {ray: (distance, slot hit or None)})]: the answers are worked out by hand from
    ORIGIN = (0.25, 0.5) and the rays +x, +y, -x, -y; every number is exactly representable."""
    s0, n = c.layer_slots['shapes']
    P = c.program
    free = [s for s in range(s0, s0 + n) if P.slot_vcap[s] >= 4]
    assert len(free) >= 3
    a, b, d = free[:3]
    nan = float('nan')
    far = float(np.nextafter(1.0, 2))   # 1.0000000000000002: its distance from y = 0.5 is one ulp above 0.5
    cases = [
        ('square ahead', {b: (box(0.75, 0.25, 1.0, 0.75), 255)}, {}, {0: (0.5, b), 1: (2.0, None), 2: (2.0, None)}),
        ('through a shared vertex', {a: ([(0.75, 0.5), (1.0, 0.75), (1.25, 0.5), (1.0, 0.25)], 255)}, {}, {0: (0.5, a)}),
        ('collinear edge', {a: (box(0.75, 0.5, 1.0, 0.75), 255)}, {}, {0: (0.5, a)}),
        ('origin inside', {a: (box(0.0, 0.25, 1.0, 0.75), 255)}, {}, {0: (0.75, a), 1: (0.25, a), 2: (0.25, a), 3: (0.25, a)}),
        ('equal distance', {b: (box(0.75, 0.25, 1.0, 0.75), 255), a: (box(0.75, 0.0, 1.5, 1.0), 255)}, {}, {0: (0.5, a)}),
        ('equal distance, rows swapped', {a: (box(0.75, 0.25, 1.0, 0.75), 255), d: (box(0.75, 0.0, 1.5, 1.0), 255)}, {}, {0: (0.5, a)}),
        ('at and beyond max_range', {a: (box(0.75, 0.25, 1.0, 0.75), 255), b: (box(0.0, far, 0.5, 1.5), 255)},
         dict(max_range=0.5), {0: (0.5, a), 1: (0.5, None)}),
        ('beyond is in reach of a longer ray', {b: (box(0.0, far, 0.5, 1.5), 255)}, dict(max_range=0.75), {1: (far - 0.5, b)}),
        ('all NaN', {a: ([(nan, nan)] * 4, 255), b: (box(1.0, 0.25, 1.25, 0.75), 255)}, {}, {0: (0.75, b)}),
        ('one NaN vertex, its edges gone', {a: ([(nan, nan), (1.0, 0.25), (1.0, 0.75), (0.75, 0.75)], 255)}, {}, {0: (0.75, a)}),
        ('one NaN vertex, the others hit', {a: ([(0.75, 0.25), (nan, 0.25), (1.0, 0.75), (0.75, 0.75)], 255)}, {}, {0: (0.5, a)}),
        ('dead origin', {a: (box(0.75, 0.25, 1.0, 0.75), 255)}, dict(origin_alive=False), {k: (2.0, None) for k in range(4)}),
        ('opacity 0, visible only', {a: (box(0.75, 0.25, 1.0, 0.75), 0), b: (box(1.0, 0.25, 1.25, 0.75), 1)}, {}, {0: (0.75, b)}),
        ('opacity 0, everything', {a: (box(0.75, 0.25, 1.0, 0.75), 0), b: (box(1.0, 0.25, 1.25, 0.75), 1)},
         dict(visible_only=False), {0: (0.5, a)}),
        ('own polygon', {}, dict(origin_verts=[(-1.0, -1.0), (2.0, 0.5), (-1.0, 2.0)]), {k: (2.0, None) for k in range(4)}),
        ('one vertex', {a: ([(0.75, 0.5)], 255)}, {}, {0: (2.0, None)}),
        ('two vertices', {a: ([(0.75, 0.25), (0.75, 0.75)], 255)}, {}, {0: (0.5, a), 2: (2.0, None)}),
        ('below, through a corner', {a: (box(0.25, 0.0, 0.5, 0.25), 255)}, {}, {3: (0.25, a), 0: (2.0, None)}),
    ]
    out = []
    for name, sprites, kw, want in cases:
        rec = {k: kw.pop(k) for k in ('origin_alive', 'origin_verts') if k in kw}
        f, q = plant(c, sprites, **rec)
        out.append((name, f, q, kw, want))
    return out


def check_planted(name, got, want, T):
    dt = sensor_dtype(T)
    for ray, (dist, slot) in want.items():
        assert got[ray, 0] == dt.type(dist) and got[ray, 1] == (0 if slot is None else slot + 1), (name, ray, got[ray], dist, slot)


@pytest.fixture(scope='module')
def zoo():
    return compile_with('ray_zoo', {})


def test_known_answers_on_planted_records(model, zoo):
    for dtype in (F32, F16):
        for name, f, q, kw, want in planted_cases(zoo):
            T = planted_sensor(zoo, dtype=dtype, **kw)
            got, = model_cast(model, zoo.program, [T], f[None], q[None])
            check_planted(name, got[0], want, T)
            assert same_bits(got, numpy_cast(zoo, T, f[None], q[None])), name
    # layer mode: what was hit is the position of the slot's layer among the rows' layers
    name, f, q, kw, want = planted_cases(zoo)[0]
    T = planted_sensor(zoo, mode=_abi.MOOG_SENSOR_LAYER)
    got, = model_cast(model, zoo.program, [T], f[None], q[None])
    assert got[0, 0, 0] == 0.5 and got[0, 0, 1] == 1 + list(zoo.layer_names).index('shapes')


@pytest.mark.parametrize('name', RECORDINGS)
def test_model_against_numpy_on_the_recordings(model, name):
    """Every recorded call, four sensors in one launch (both modes, both dtypes; 7, 32, 65 and 256 rays): bit for bit."""
    sensors = recording_sensors(name)
    c = compile_with(name, sensors)
    assert [k for k, _ in c.sensors] == list(sensors)
    fx, f64, i32 = fixture_records(name, c)
    T = [t for _, t in c.sensors]
    got = model_cast(model, c.program, T, f64, i32)
    hits = 0
    for k, t in enumerate(T):
        want = numpy_cast(c, t, f64, i32)
        assert same_bits(got[k], want), (name, k, np.argwhere(bits(got[k]) != bits(want))[:5])
        hits += int((got[k][:, :, 1] != 0).sum())
    assert hits > 0
    # the edge-chunk boundary: chunks of 7 edges, and of 1, give the bits of one chunk of 128
    for chunk in (7, 1):
        again = model_cast(model, c.program, T, f64[:6], i32[:6], chunk=chunk)
        for k in range(len(T)):
            assert same_bits(again[k], got[k][:6]), (name, chunk, k)
    if name == 'falling_balls_64':   # (more edges than one chunk holds: the several-chunk path at the kernel's own size)
        L, S = c.layout, c.layout.S
        live = (i32[:, L.o_flags:L.o_flags + S] & _abi.MOOG_F_ALIVE) != 0
        assert int((i32[:, L.o_nverts:L.o_nverts + S] * live).sum(axis=1).max()) > model.rs_model_chunk()


def test_follow_angle_on_ray_zoo(model, zoo):
    """With the model fed numpy's cos / sin the rotated fan equals the numpy implementation bit for bit, and the rays whose
    id an angle change of 1e-12 rad flips (the ones a device's own cos / sin may decide differently) are at most 1 %."""
    f64, i32 = zoo_states(zoo)
    L, a = zoo.layout, zoo.layer_slots['agent'][0]
    ang = f64[:, L.o_angle + a]
    assert np.all(np.abs(ang / (np.pi / 8) - np.round(ang / (np.pi / 8))) > 1e-6)   # no multiple of pi / 8
    obs = {'f': observers.RaySensor('agent', num_rays=64, follow_angle=True, max_range=1.5),
           'g': observers.RaySensor('agent', num_rays=16, fov=np.pi / 2, follow_angle=True, max_range=0.75, mode='layer',
                                    visible_only=False, dtype='float16')}
    c = compile_with('ray_zoo', obs)
    assert bytes(c.program) == bytes(zoo.program)
    T = [t for _, t in c.sensors]
    ex, base = excused_rays(model, c, T, f64, i32)
    cs = cos_sin(c, T, f64)
    for k, t in enumerate(T):
        assert same_bits(base[k], numpy_cast(c, t, f64, i32, cs=cs[k])), k
    n_ex, n_all = sum(int(e.sum()) for e in ex), sum(e.size for e in ex)
    print('follow_angle: %d of %d rays excused' % (n_ex, n_all))
    assert n_ex <= 0.01 * n_all
    assert sum(int((b[:, :, 1] != 0).sum()) for b in base) > n_all // 2


def test_lowering_rows_and_spec():
    sensors = {'r': observers.RaySensor('agent', num_rays=5, layers=('shapes', 'prey'), max_range=0.5),
               'l': observers.RaySensor('agent', layers=('prey', 'walls'), mode='layer', follow_angle=True, dtype='float16',
                                        visible_only=False)}
    sensors['t'] = observers.SpriteTable(layers=('shapes', 'prey'))
    c = compile_with('ray_zoo', sensors)
    T = dict(c.sensors)
    s_sh, n_sh = c.layer_slots['shapes']
    s_pr, n_pr = c.layer_slots['prey']
    assert n_pr == 24
    assert c.sensor_rows['r'] == [('shapes', k) for k in range(n_sh)] + [('prey', k) for k in range(n_pr)] == c.table_rows['t']
    assert [T['r'].row_slot[k] for k in range(T['r'].n_rows)] == list(range(s_sh, s_sh + n_sh)) + list(range(s_pr, s_pr + n_pr))
    assert T['r'].origin_slot == c.layer_slots['agent'][0] and T['r'].flags == _abi.MOOG_SENSOR_VISIBLE_ONLY
    assert T['l'].flags == _abi.MOOG_SENSOR_FOLLOW_ANGLE and T['l'].mode == _abi.MOOG_SENSOR_LAYER and T['l'].dtype == F16
    k = np.arange(5)
    theta = np.pi / 2 + 2 * np.pi * ((k + 0.5) / 5 - 0.5)
    want = np.stack([np.cos(theta), np.sin(theta)], axis=1)
    assert np.array_equal(np.array([[T['r'].dirs[i][0], T['r'].dirs[i][1]] for i in range(5)]), want)
    assert np.array_equal(sensors['r'].directions, want)
    spec = sensors['r'].observation_spec()
    assert spec.shape == (5, 2) and spec.dtype == np.float32
    assert sensors['l'].observation_spec().shape == (32, 2) and sensors['l'].observation_spec().dtype == np.float16
    # never part of the program
    assert bytes(c.program) == bytes(compile_with('ray_zoo', {}).program)
    # the demo config's own sensors
    full = _compiler.compile_config(layer_capacity=example_configs.capacity('ray_zoo'), **example_configs.load('ray_zoo'))
    assert [k for k, _ in full.sensors] == ['rays', 'front'] and full.sensor_rows['rays'] == full.table_rows['table']


def test_python_refusals():
    R = observers.RaySensor
    for kw, word in ((dict(num_rays=0), 'num_rays'), (dict(num_rays=257), 'num_rays'), (dict(max_range=0.0), 'max_range'),
                     (dict(max_range=float('inf')), 'max_range'), (dict(max_range=float('nan')), 'max_range'),
                     (dict(max_range=70000.0, dtype='float16'), '65504'), (dict(fov=0.0), 'fov'), (dict(fov=6.3), 'fov'),
                     (dict(mode='pixel'), 'mode'), (dict(dtype='float64'), 'dtype'), (dict(layers=('prey', 'prey')), 'twice'),
                     (dict(heading=float('inf')), 'finite')):
        with pytest.raises(ValueError, match=word):
            R('agent', **kw)
    R('agent', max_range=70000.0)   # (float32 holds it)
    for sensor, exc, word in ((R('agent', layers=('nowhere',)), ValueError, 'unknown layer'),
                              (R('nobody'), ValueError, 'origin_layer'),
                              (R('agent', origin_index=1), ValueError, 'origin_index')):
        with pytest.raises(exc, match=word):
            compile_with('ray_zoo', {'s': sensor})
    with pytest.raises(NotImplementedError, match='MOOG_MAX_SENSORS'):
        compile_with('ray_zoo', {'s%d' % k: R('agent') for k in range(_abi.MOOG_MAX_SENSORS + 1)})
    # more than 255 rows in instance mode; layer mode takes them
    cfg = example_configs.load('ray_zoo')
    base = compile_with('ray_zoo', {}).layout.S
    for mode, ok in (('instance', False), ('layer', True)):
        cfg['observers'] = {'s': R('agent', mode=mode)}
        make = lambda: _compiler.compile_config(layer_capacity={'prey': 256 - (base - 24)}, **cfg)
        if ok:
            assert dict(make().sensors)['s'].n_rows == 256
        else:
            with pytest.raises(NotImplementedError, match='255'):
                make()


def test_model_refuses_what_the_engine_refuses(model, zoo):
    """moog_rs_describe is the engine's check (moog_engine_add_sensor)."""
    f, q = plant(zoo, {})
    good = planted_sensor(zoo)
    model_cast(model, zoo.program, [good], f[None], q[None])
    for edit, word in ((lambda T: setattr(T, 'n_rays', 0), 'n_rays'), (lambda T: setattr(T, 'n_rays', 257), 'n_rays'),
                       (lambda T: setattr(T, 'max_range', 0.0), 'max_range'), (lambda T: setattr(T, 'max_range', float('nan')), 'max_range'),
                       (lambda T: setattr(T, 'max_range', float('inf')), 'max_range'),
                       (lambda T: (setattr(T, 'max_range', 65505.0), setattr(T, 'dtype', F16)), '65504'),
                       (lambda T: setattr(T, 'mode', 2), 'mode'), (lambda T: setattr(T, 'dtype', 2), 'dtype'),
                       (lambda T: setattr(T, 'flags', 4), 'flag'), (lambda T: setattr(T, 'origin_slot', zoo.layout.S), 'origin'),
                       (lambda T: T.row_slot.__setitem__(1, zoo.layout.S), 'slot'), (lambda T: T.row_slot.__setitem__(1, 0), 'two rows'),
                       (lambda T: setattr(T, 'n_rows', 0), 'n_rows'),
                       (lambda T: T.dirs[3].__setitem__(1, float('nan')), 'direction'), (lambda T: T.dirs[0].__setitem__(0, float('inf')), 'direction')):
        T = _abi.Sensor.from_buffer_copy(good)
        edit(T)
        with pytest.raises(ValueError, match=word):
            model_cast(model, zoo.program, [T], f[None], q[None])
    with pytest.raises(ValueError, match='MOOG_MAX_SENSORS'):
        model_cast(model, zoo.program, [good] * (_abi.MOOG_MAX_SENSORS + 1), f[None], q[None])


def test_abi_is_additive():
    assert _abi.MOOG_ABI_VERSION == 31 and _abi.MOOG_PROGRAM_VERSION == 30 and _abi.MOOG_K_COUNT == 5
    assert _abi.MOOG_MAX_RAYS == 256 and _abi.MOOG_MAX_SENSORS == 4
    import re
    with open(_abi.HEADER) as fh:
        declared = set(re.findall(r'\b(moog_\w+)\s*\(', fh.read())) - {'moog_layout', 'moog_align_'}
    for sym in ('moog_engine_add_sensor', 'moog_engine_set_sensor_buffer', 'moog_engine_observe_sensors'):
        assert sym in _engine.SYMBOLS and sym in declared, sym
    assert declared == set(_engine.SYMBOLS), declared ^ set(_engine.SYMBOLS)
    assert ctypes.sizeof(_abi.Sensor) == 6 * 4 + 8 + 4 * _abi.MOOG_MAX_SLOTS + 16 * _abi.MOOG_MAX_RAYS
