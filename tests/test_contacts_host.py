"""Contacts observer without a GPU: the host model of the contacts kernel (csrc/moog_contacts.h compiled with g++ -O2
-ffp-contract=off, tests/csrc/contacts_model.cpp: the descriptors and the wave function the kernel runs, walked lane by lane)
against the matrices recorded with matplotlib (tests/golden/contacts_<name>_s0.npz, exact, no pair left out), against an
independent formulation -- the oracle's oracle_paths_intersect behind the circle test, in a plain double loop -- on
oracle-stepped and planted records, with the candidate chunk size varied; the lowering, the refusals and the spec.  The
kernel itself is held to the same expectations by tests/test_contacts_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers
from moog import _abi
from moog import _compiler
from moog import observers
from moog.observers import contacts as contacts_lib
from moog_demos import example_configs

SRC = os.path.join(helpers.REPO, 'tests', 'csrc', 'contacts_model.cpp')
RECORDINGS = ('colliding_predators_32', 'falling_balls_64', 'cleanup', 'pong')
# (calls, ordered live pairs, past the circle, overlapping) as measured with matplotlib when the observer was specified
COUNTS = {'colliding_predators_32': (41, 40672, 4542, 446), 'falling_balls_64': (13, 52416, 2612, 78),
          'cleanup': (151, 140430, 12820, 2308), 'pong': (97, 1812, 1394, 436)}
PAIR, LAYER, VISIBLE = _abi.MOOG_CONTACTS_PAIR, _abi.MOOG_CONTACTS_LAYER, _abi.MOOG_CONTACTS_VISIBLE_ONLY


def build_model():
    return helpers.build_host_model(SRC, 'contacts_model')


@pytest.fixture(scope='module')
def model():
    return build_model()


def model_shape(m, P, T):
    """(n0, n1, n_layers_1, same) as the header's describe function sees a description; ValueError with its refusal."""
    shape = (ctypes.c_int32 * 4)()
    err = ctypes.create_string_buffer(256)
    if m.ct_model_shape(ctypes.byref(P), ctypes.byref(T), shape, err, 256) != 0:
        raise ValueError(err.value.decode())
    return tuple(shape)


def model_observe(m, P, descs, f64, i32, chunk=0, offset=0, cands=False):
    """One model launch over host records: [uint8 [n, R0, R1 or layers] per observer] (and [observers, n] candidate counts).
    offset: the byte of a dword every buffer starts at."""
    n = f64.shape[0]
    arr = (_abi.Contacts * len(descs))(*descs)
    outs = []
    for T in descs:
        n0, n1, nl, _ = model_shape(m, P, T)
        shape = (n, n0, nl if T.mode == LAYER else n1)
        raw = np.full(int(np.prod(shape)) + 16, 0x55, np.uint8)
        start = (-raw.ctypes.data) % 4 + offset
        outs.append((raw, start, shape))
    ptrs = (ctypes.c_void_p * len(descs))(*[raw.ctypes.data + start for raw, start, _ in outs])
    err = ctypes.create_string_buffer(256)
    f64, i32 = np.ascontiguousarray(f64, np.float64), np.ascontiguousarray(i32, np.int32)
    nc = np.zeros((len(descs), n), np.int32)
    rc = m.ct_model_observe(ctypes.byref(P), arr, len(descs), f64.ctypes.data_as(ctypes.c_void_p),
                            i32.ctypes.data_as(ctypes.c_void_p), n, ptrs, int(chunk), nc.ctypes.data_as(ctypes.c_void_p), err, 256)
    if rc != 0:
        raise ValueError(err.value.decode())
    res = []
    for raw, start, shape in outs:
        count = int(np.prod(shape))
        assert np.all(raw[:start] == 0x55) and np.all(raw[start + count:] == 0x55)   # nothing outside the tensor
        res.append(raw[start:start + count].reshape(shape).copy())
    return (res, nc) if cands else res


# ---- the independent formulation -------------------------------------------------------------------------------------
def slot_overlaps(P, L, f, q, visible_only=False):
    """[S, S] uint8 over one record: the rule of the Contacts docstring for every ordered pair of slots, in a plain double loop
    -- the circle test (the oracle's npnorm: sqrt(fma(dy, dy, dx * dx))), then oracle_paths_intersect."""
    lib = helpers.oracle()
    lib.oracle_npnorm.restype = ctypes.c_double
    lib.oracle_npnorm.argtypes = [ctypes.c_double, ctypes.c_double]
    dp = ctypes.POINTER(ctypes.c_double)
    S = L.S
    out = np.zeros((S, S), np.uint8)
    ok = [bool(q[L.o_flags + s] & _abi.MOOG_F_ALIVE) and (not visible_only or q[L.o_opacity + s] > 0) for s in range(S)]
    verts = {}
    for s in range(S):
        if ok[s]:
            n = max(0, min(int(q[L.o_nverts + s]), int(P.slot_vcap[s])))
            o = L.o_verts + 2 * P.slot_voff[s]
            verts[s] = (np.ascontiguousarray(f[o:o + 2 * max(n, 1)], np.float64), n)
    for a in range(S):
        for b in range(S):
            if a == b or not ok[a] or not ok[b]:
                continue
            dx, dy = f[L.o_pos + 2 * a] - f[L.o_pos + 2 * b], f[L.o_pos + 2 * a + 1] - f[L.o_pos + 2 * b + 1]
            if lib.oracle_npnorm(float(dx), float(dy)) > f[L.o_maxr + a] + f[L.o_maxr + b]:
                continue
            (va, na), (vb, nb) = verts[a], verts[b]
            out[a, b] = lib.oracle_paths_intersect(va.ctypes.data_as(dp), na, vb.ctypes.data_as(dp), nb)
    return out


def expected(P, T, slot_matrix):
    """What observer T shows for a record whose [S, S] slot matrix is given."""
    r0 = [T.row_slot_0[k] for k in range(T.n_rows_0)]
    r1 = [T.row_slot_1[k] for k in range(T.n_rows_1)]
    pair = slot_matrix[np.ix_(r0, r1)]
    if T.mode == PAIR:
        return pair
    cols, last = [], None
    for j, s in enumerate(r1):
        if P.slot_layer[s] != last:
            cols.append([])
            last = P.slot_layer[s]
        cols[-1].append(j)
    return np.stack([pair[:, c].max(axis=1) for c in cols], axis=1)


def check_records(m, c, descs, f64, i32, matrices=None, **kw):
    """Model against the double loop (or the given slot matrices) for every env; returns the model's tensors."""
    P, L = c.program, c.layout
    got = model_observe(m, P, descs, f64, i32, **kw)
    for k, T in enumerate(descs):
        for e in range(f64.shape[0]):
            M = matrices[e] if matrices is not None else slot_overlaps(P, L, f64[e], i32[e], bool(T.flags & VISIBLE))
            want = expected(P, T, M)
            assert np.array_equal(got[k][e], want), ('observer %d, env %d' % (k, e), np.argwhere(got[k][e] != want)[:8])
    return got


# ---- configs and records ---------------------------------------------------------------------------------------------
def compile_with(name, extra, alone=False):
    cfg = example_configs.load(name)
    obs = {} if alone else dict(cfg['observers'])
    obs.update(extra)
    cfg['observers'] = obs
    return _compiler.compile_config(layer_capacity=example_configs.capacity(name), **cfg)


def fixture_records(name, c):
    fx = helpers.fixture(name, 0)
    n = len(fx['step_type'])
    f64 = np.zeros((n, c.layout.f64_per_env))
    i32 = np.zeros((n, c.layout.i32_per_env), np.int32)
    for t in range(n):
        helpers.records_from_fixture(fx, t, c, f64, i32, env=t)
    return fx, f64, i32


def recorded_matrices(name):
    with np.load(os.path.join(helpers.GOLDEN, 'contacts_%s_s0.npz' % name)) as z:
        S = int(z['n_slots'])
        bits, counts = z['bits'], tuple(int(v) for v in z['counts'])
    M = np.unpackbits(bits, axis=1)[:, :S * S].reshape(-1, S, S)
    return M, counts


def layers_with_slots(name):
    c = helpers.compiled(name)
    return [k for k in c.layer_names if c.layer_slots[k][1] > 0]


def recording_observers(name):
    names = layers_with_slots(name)
    first = tuple(k for k in names if k.startswith('agent_')) if name == 'cleanup' else tuple(names[-1:])   # cleanup's agents
    rest = tuple(k for k in names if k not in first) or first
    return {'all': observers.Contacts(tuple(names)),
            'all_l': observers.Contacts(tuple(names), mode='layer'),
            'rect': observers.Contacts(first, rest),
            'rect_l': observers.Contacts(rest, tuple(names), mode='layer')}


@pytest.mark.parametrize('name', RECORDINGS)
def test_model_equals_the_recorded_matrices(model, name):
    """Teacher-forced, one env per recorded call: both modes, layers_1=None and rectangular choices, exact, every pair."""
    c = compile_with(name, recording_observers(name))
    M, counts = recorded_matrices(name)
    assert (M.shape[0],) + counts == COUNTS[name]
    assert int(M.sum()) == counts[2]
    fx, f64, i32 = fixture_records(name, c)
    assert M.shape[0] == f64.shape[0] and M.shape[1] == c.layout.S
    descs = [T for _, T in c.contacts]
    assert model_shape(model, c.program, descs[0])[3] == 1 and model_shape(model, c.program, descs[2])[3] == 0
    got = check_records(model, c, descs, f64, i32, matrices=M)
    assert int(got[0].sum()) == counts[2]   # (every slot is a row of 'all': nothing is left out)


def zoo_states(c, n=24, steps=6, seed=11):
    o = helpers.OracleEnv(c, n_envs=n, seed=seed)
    o.reset(render=False)
    rs = np.random.RandomState(seed)
    for _ in range(steps):
        o.step(rs.uniform(-1, 1, size=(n, 2)), render=False)
    return o.f64.copy(), o.i32.copy()


ZOO = {'pair': dict(layers_0=('walls', 'shapes', 'prey', 'agent')),
       'odd': dict(layers_0=('shapes',), layers_1=('shapes', 'walls'), visible_only=True),   # 7 x 11 bytes an env
       'layer': dict(layers_0=('agent', 'prey'), layers_1=('walls', 'shapes', 'prey', 'agent'), mode='layer'),
       'layer_sq': dict(layers_0=('shapes', 'agent'), mode='layer', visible_only=True)}


def zoo_compiled():
    return compile_with('ray_zoo', {k: observers.Contacts(**kw) for k, kw in ZOO.items()})


def test_model_equals_the_double_loop_on_ray_zoo(model):
    c = zoo_compiled()
    f64, i32 = zoo_states(c)
    descs = [T for _, T in c.contacts]
    got = check_records(model, c, descs, f64, i32)
    assert got[0].any() and got[2].any()
    assert np.array_equal(got[0], np.stack([expected(c.program, descs[0], slot_overlaps(c.program, c.layout, f64[e], i32[e]))
                                            for e in range(f64.shape[0])]))
    for off in (1, 2, 3):   # a block may start at any byte
        again = model_observe(model, c.program, descs, f64, i32, offset=off)
        assert all(np.array_equal(a, b) for a, b in zip(again, got))


# ---- planted records -------------------------------------------------------------------------------------------------
def synthetic(c, vcap=128):
    """The compiled program on a synthetic layout: every slot with room for `vcap` vertices."""
    P = _abi.Program.from_buffer_copy(bytes(c.program))
    S = c.layout.S
    for s in range(S):
        P.slot_vcap[s] = vcap
        P.slot_voff[s] = s * vcap
    P.n_total_verts = S * vcap
    return c._replace(program=P, layout=_abi.layout_of(P))


def blank(c, n=1):
    return np.zeros((n, c.layout.f64_per_env)), np.zeros((n, c.layout.i32_per_env), np.int32)


def plant(c, f64, i32, slot, verts, env=0, pos=None, maxr=None, opacity=255, alive=True, nverts=None):
    P, L = c.program, c.layout
    v = np.asarray(verts, np.float64).reshape(-1, 2)
    f, q = f64[env], i32[env]
    o = L.o_verts + 2 * P.slot_voff[slot]
    f[o:o + 2 * len(v)] = v.ravel()
    p = np.nanmean(v, axis=0) if pos is None else np.asarray(pos, np.float64)
    if pos is None and not np.all(np.isfinite(p)):
        p = np.array([0.5, 0.5])
    f[L.o_pos + 2 * slot:L.o_pos + 2 * slot + 2] = p
    with np.errstate(invalid='ignore'):
        r = np.nanmax(np.hypot(v[:, 0] - p[0], v[:, 1] - p[1]), initial=0.0) * 1.001 + 1e-9
    f[L.o_maxr + slot] = r if maxr is None else maxr
    q[L.o_flags + slot] = _abi.MOOG_F_ALIVE if alive else 0
    q[L.o_nverts + slot] = len(v) if nverts is None else nverts
    q[L.o_opacity + slot] = opacity


def box(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def all_slots(c, mode=PAIR, flags=0, rows_1=None):
    S = c.layout.S
    T = _abi.Contacts()
    T.n_rows_0, T.mode, T.flags = S, mode, flags
    rows_1 = list(range(S)) if rows_1 is None else rows_1
    T.n_rows_1 = len(rows_1)
    for s in range(S):
        T.row_slot_0[s] = s
    for k, s in enumerate(rows_1):
        T.row_slot_1[k] = s
    return T


def planted_scenes(c):
    """(f64, i32, {env: {(a, b): answer}}): one scene per env on the synthetic layout of `c` (slots 0 .. 3 are used)."""
    scenes = []
    # 0: two squares sharing only an edge; 1: sharing only a corner
    scenes.append(([(0, box(0.2, 0.2, 0.4, 0.4)), (1, box(0.4, 0.2, 0.6, 0.4))], {}, {(0, 1): 1, (1, 0): 1}))
    scenes.append(([(0, box(0.2, 0.2, 0.4, 0.4)), (1, box(0.4, 0.4, 0.6, 0.6))], {}, {(0, 1): 1, (1, 0): 1}))
    # 2: one strictly inside the other, both orders
    scenes.append(([(0, box(0.2, 0.2, 0.8, 0.8)), (1, box(0.4, 0.4, 0.5, 0.5))], {}, {(0, 1): 1, (1, 0): 1}))
    # 3: a concave polygon whose notch holds the other without touching
    cee = [(0.2, 0.2), (0.8, 0.2), (0.8, 0.3), (0.3, 0.3), (0.3, 0.7), (0.8, 0.7), (0.8, 0.8), (0.2, 0.8)]
    scenes.append(([(0, cee), (1, box(0.45, 0.45, 0.55, 0.55))], {}, {(0, 1): 0, (1, 0): 0}))
    # 4 / 5: overlapping squares whose circles touch to the last ulp (norm == r0 + r1: not apart), and one ulp less
    sq = box(0.4, 0.4, 0.6, 0.6)
    scenes.append(([(0, sq), (1, sq)], {0: dict(pos=(0.0, 0.0), maxr=0.5), 1: dict(pos=(1.0, 0.0), maxr=0.5)},
                   {(0, 1): 1, (1, 0): 1}))
    # (both radii one ulp down: their sum is the double below 1.0 exactly; one alone would round back up to 1.0)
    below = np.nextafter(0.5, 0.0)
    scenes.append(([(0, sq), (1, sq)], {0: dict(pos=(0.0, 0.0), maxr=below), 1: dict(pos=(1.0, 0.0), maxr=below)},
                   {(0, 1): 0, (1, 0): 0}))
    # 6: a dead row; 7: an opacity-0 row (seen unless visible_only)
    scenes.append(([(0, sq), (1, sq), (2, sq)], {1: dict(alive=False)}, {(0, 1): 0, (1, 0): 0, (0, 2): 1, (2, 1): 0}))
    scenes.append(([(0, sq), (1, sq), (2, sq)], {1: dict(opacity=0)}, {(0, 1): 1, (1, 2): 1, (0, 2): 1}))
    # 8: a sprite whose vertices are all NaN overlaps every live row whose circle it reaches (position and radius are finite)
    nan = [(np.nan, np.nan)] * 4
    scenes.append(([(0, nan), (1, box(0.1, 0.1, 0.2, 0.2)), (2, box(0.7, 0.7, 0.9, 0.9)), (3, sq)],
                   {0: dict(pos=(0.5, 0.5), maxr=2.0), 3: dict(alive=False)},
                   {(0, 1): 1, (1, 0): 1, (0, 2): 1, (2, 0): 1, (1, 2): 0, (0, 3): 0}))
    # 9: nverts above the capacity is cut to the capacity (128 here): the square is the first four of 128 equal... a 128-gon
    th = 2 * np.pi * np.arange(128) / 128
    big = np.stack([0.5 + 0.3 * np.cos(th), 0.5 + 0.3 * np.sin(th)], axis=1)
    scenes.append(([(0, big), (1, box(0.75, 0.45, 0.9, 0.55)), (2, box(0.85, 0.85, 0.95, 0.95))], {0: dict(nverts=1000)},
                   {(0, 1): 1, (1, 0): 1, (0, 2): 0}))
    # 10: a collinear-overlap pair for which the two orders differ: a's short bottom edge lies 5e-11 above b's long top edge
    # -- twice the triangle's area is 5e-14 measured from a's edge (isclose to 0: collinear, the x ranges overlap) and 5e-11
    # measured from b's (parallel, apart)
    scenes.append(([(0, [(0.4, 0.0), (0.401, 0.0), (0.401, 0.1), (0.4, 0.1)]), (1, [(0.0, -1.0), (1.0, -1.0), (1.0, -5e-11), (0.0, -5e-11)])],
                   {}, {(0, 1): 1, (1, 0): 0}))
    # 11: polygons of more than 64 vertices: a 100-gon star crossing a 90-gon ring's edge, and one inside the other
    th = 2 * np.pi * np.arange(100) / 100
    star = np.stack([0.5 + (0.2 + 0.05 * (np.arange(100) % 2)) * np.cos(th), 0.5 + (0.2 + 0.05 * (np.arange(100) % 2)) * np.sin(th)], axis=1)
    th = 2 * np.pi * np.arange(90) / 90
    ring = np.stack([0.72 + 0.1 * np.cos(th), 0.5 + 0.1 * np.sin(th)], axis=1)
    small = np.stack([0.5 + 0.05 * np.cos(th), 0.5 + 0.05 * np.sin(th)], axis=1)
    scenes.append(([(0, star), (1, ring), (2, small)], {}, {(0, 1): 1, (1, 0): 1, (0, 2): 1, (2, 0): 1, (1, 2): 0}))
    f64, i32 = blank(c, len(scenes))
    answers = {}
    for e, (sprites, kw, ans) in enumerate(scenes):
        for slot, verts in sprites:
            plant(c, f64, i32, slot, verts, env=e, **kw.get(slot, {}))
        answers[e] = ans
    return f64, i32, answers


def test_planted_records(model):
    c = synthetic(helpers.compiled('colliding_predators_32'))
    assert c.layout.S >= 4
    f64, i32, answers = planted_scenes(c)
    descs = [all_slots(c), all_slots(c, flags=VISIBLE), all_slots(c, mode=LAYER),
             all_slots(c, rows_1=[1, 0, 3, 2])]   # (a slot in both arguments, rectangular: the diagonal moves)
    got = check_records(model, c, descs, f64, i32)
    for e, ans in answers.items():
        for (a, b), v in ans.items():
            assert got[0][e, a, b] == v, ('scene %d pair (%d, %d)' % (e, a, b), got[0][e, :4, :4])
    S = c.layout.S
    assert not got[0][:, np.arange(S), np.arange(S)].any()   # the diagonal: one slot
    assert not got[3][:, [1, 0, 3, 2], [0, 1, 2, 3]].any()     # and where the same slot stands in a rectangular choice
    assert got[3][0, 0, 0] == 1                                # (row 0 against slot 1)
    assert got[1][7, 0, 1] == 0 and got[1][7, 1, 2] == 0 and got[1][7, 0, 2] == 1   # visible_only drops the opacity-0 row
    assert got[0][10, 0, 1] == 1 and got[0][10, 1, 0] == 0     # the two orders, each on its own


def test_chunk_independence(model):
    """Candidate chunk sizes 1, 3 and the kernel's own give identical bytes."""
    own = model.ct_model_chunk()
    cases = []
    c = synthetic(helpers.compiled('colliding_predators_32'))
    f64, i32, _ = planted_scenes(c)
    cases.append((c, [all_slots(c), all_slots(c, mode=LAYER), all_slots(c, rows_1=[1, 0, 3, 2])], f64, i32))
    for name in ('falling_balls_64', 'cleanup'):
        cc = compile_with(name, recording_observers(name))
        _, f64, i32 = fixture_records(name, cc)
        cases.append((cc, [T for _, T in cc.contacts], f64[::3], i32[::3]))
    for cc, descs, f64, i32 in cases:
        ref, nc = model_observe(model, cc.program, descs, f64, i32, cands=True)
        assert nc.max() > 3
        for chunk in (1, 3, own):
            got, nc2 = model_observe(model, cc.program, descs, f64, i32, chunk=chunk, cands=True)
            assert np.array_equal(nc, nc2)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref)), chunk
    with pytest.raises(ValueError, match='chunk above MOOG_CT_CHUNK'):
        model_observe(model, cc.program, descs, f64, i32, chunk=own + 1)


# ---- lowering --------------------------------------------------------------------------------------------------------
def test_rows_are_sprite_table_rows_and_spec():
    obs = {k: observers.Contacts(**kw) for k, kw in ZOO.items()}
    obs['t0'] = observers.SpriteTable(layers=('shapes',), columns=('alive',))
    obs['t1'] = observers.SpriteTable(layers=('shapes', 'walls'), columns=('alive',))
    c = compile_with('ray_zoo', obs)
    assert [k for k, _ in c.contacts] == list(ZOO)
    rows_0, rows_1 = c.contact_rows['odd']
    assert rows_0 == c.table_rows['t0'] and rows_1 == c.table_rows['t1']
    T = dict(c.contacts)
    assert [T['odd'].row_slot_0[k] for k in range(T['odd'].n_rows_0)] == [dict(c.tables)['t0'].row_slot[k] for k in range(len(rows_0))]
    assert [T['odd'].row_slot_1[k] for k in range(T['odd'].n_rows_1)] == [dict(c.tables)['t1'].row_slot[k] for k in range(len(rows_1))]
    assert c.contact_rows['pair'][0] == c.contact_rows['pair'][1] == c.table_rows['table']
    n = {k: c.layer_slots[k][1] for k in c.layer_names}
    shapes = {'pair': (36, 36), 'odd': (n['shapes'], n['shapes'] + n['walls']), 'layer': (n['agent'] + n['prey'], 4),
              'layer_sq': (n['shapes'] + n['agent'], 2)}
    for key, o in obs.items():
        if key in ZOO:
            spec = contacts_lib.contacts_spec(T[key])
            assert spec.shape == shapes[key] and spec.dtype == np.uint8
            assert o.observation_spec().shape == shapes[key] and o.observation_spec().dtype == np.uint8
    assert T['odd'].flags == VISIBLE and T['pair'].flags == 0 and T['layer'].mode == LAYER and T['pair'].mode == PAIR
    assert (shapes['odd'][0] * shapes['odd'][1]) % 2 == 1
    with pytest.raises(ValueError, match='build the environment first'):
        observers.Contacts('agent').observation_spec()


def test_configs_without_contacts_compile_to_the_same_program():
    for name in ('ray_zoo', 'colliding_predators_32'):
        plain = compile_with(name, {})
        layers = tuple(layers_with_slots(name))
        with_c = compile_with(name, {'touch': observers.Contacts(layers), 'touch_l': observers.Contacts(layers[-1], layers, mode='layer')})
        assert bytes(plain.program) == bytes(with_c.program)
        assert plain.contacts == [] and plain.contact_rows == {} and len(with_c.contacts) == 2
        assert [k for k, _ in plain.tables] == [k for k, _ in with_c.tables]


def test_refusals_on_the_host(model):
    with pytest.raises(ValueError, match="unknown mode 'both'"):
        observers.Contacts('agent', mode='both')
    with pytest.raises(ValueError, match='a layer is named twice in layers_0'):
        observers.Contacts(('agent', 'agent'))
    with pytest.raises(ValueError, match='a layer is named twice in layers_1'):
        observers.Contacts('agent', ('walls', 'prey', 'walls'))
    with pytest.raises(ValueError, match="unknown layer 'ghosts' in layers_1"):
        compile_with('ray_zoo', {'c': observers.Contacts('agent', ('walls', 'ghosts'))})
    with pytest.raises(ValueError, match="unknown layer 'ghosts' in layers_0"):
        compile_with('ray_zoo', {'c': observers.Contacts('ghosts')})
    five = {'c%d' % k: observers.Contacts('agent', 'walls') for k in range(5)}
    with pytest.raises(NotImplementedError, match=r'at most 4 Contacts observers per config \(MOOG_MAX_CONTACTS\), got 5'):
        compile_with('ray_zoo', five)
    # a layer without a sprite slot: 0 rows
    cfg = example_configs.load('ray_zoo')
    cfg['observers'] = {'c': observers.Contacts('prey')}
    with pytest.raises(ValueError, match=r'the layers of layers_0 hold no sprite slot \(0 rows\)'):
        _compiler.compile_config(layer_capacity={'prey': 0}, **cfg)
    cfg['observers'] = {'c': observers.Contacts('agent', ('walls', 'prey'), mode='layer')}
    with pytest.raises(ValueError, match="layer 'prey' of layers_1 holds no sprite slot"):
        _compiler.compile_config(layer_capacity={'prey': 0}, **cfg)

    class Other(object):
        pass
    with pytest.raises(NotImplementedError, match='RaySensor and Contacts are not lowered'):
        compile_with('ray_zoo', {'x': Other()})
    # the same refusals in the header's describe function (the C ABI's, tests/test_contacts_gpu.py)
    c = helpers.compiled('colliding_predators_32')
    P = c.program

    def desc(**kw):
        T = all_slots(c)
        for k, v in kw.items():
            setattr(T, k, v)
        return T
    for kw, why in ((dict(n_rows_0=0), 'n_rows_0 outside 1 .. MOOG_MAX_SLOTS'), (dict(n_rows_1=0), 'n_rows_1 outside 1 .. MOOG_MAX_SLOTS'),
                    (dict(n_rows_0=257), 'n_rows_0 outside'), (dict(n_rows_1=257), 'n_rows_1 outside'),
                    (dict(mode=2), 'mode is neither MOOG_CONTACTS_PAIR nor MOOG_CONTACTS_LAYER'), (dict(flags=2), 'unknown flag bits')):
        with pytest.raises(ValueError, match=why):
            model_shape(model, P, desc(**kw))
    T = all_slots(c)
    T.row_slot_1[1] = T.row_slot_1[0]
    with pytest.raises(ValueError, match='a slot is named by two rows of one list'):
        model_shape(model, P, T)
    T = all_slots(c)
    T.row_slot_0[0] = c.layout.S
    with pytest.raises(ValueError, match='outside the layout'):
        model_shape(model, P, T)
    assert model_shape(model, P, all_slots(c))[:2] == (c.layout.S, c.layout.S)
