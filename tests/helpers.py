"""Shared test helpers: oracle binding, golden fixtures <-> state records.

The oracle (oracle/libmoog_oracle.so) is test infrastructure; only tests,
__graft_entry__.smoke() and bench.py's cpu_baseline leg load it.
"""
import ctypes
import functools
import glob
import os
import subprocess

import numpy as np

from moog import _abi, _compiler
from moog_demos import example_configs

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
GOLDEN = os.path.join(REPO, 'tests', 'golden')
ORACLE_DIR = os.path.join(REPO, 'oracle')
ORACLE_SO = os.path.join(ORACLE_DIR, 'libmoog_oracle.so')

# Every reference recording of tests/golden (<name>_s<seed>.npz written by tests/golden/make_golden.py): the one list both the
# oracle tests (test_oracle_golden.py) and the HIP tests (test_gpu_parity.py) are parametrised by.
# test_host.py::test_runs_list_equals_the_recordings_on_disk fails when this list and the directory differ.
RUNS = [('pong', 0), ('pong', 1), ('chase_avoid_torus', 0), ('chase_avoid_torus', 1), ('colliding_predators', 0),
        ('colliding_predators', 1), ('colliding_predators', 2), ('chase_avoid_torus', 2), ('functional_maze', 0),
        ('functional_maze', 1), ('falling_balls', 0), ('colliding_predators_32', 0), ('falling_balls_64', 0),
        ('falling_balls_64', 1), ('forces_zoo', 0), ('forces_zoo', 1), ('chase_avoid_torus_l1', 0),
        ('tether_zoo_l0', 0), ('tether_zoo_l1', 0), ('tether_zoo_l2', 0), ('tether_zoo_l3', 0), ('tether_zoo_l4', 0),
        ('distrib_zoo', 0), ('distrib_zoo', 1), ('rules_zoo_l0', 0), ('rules_zoo_l1', 0), ('rules_zoo_l1', 1),
        ('lambda_zoo', 0), ('lambda_zoo', 1), ('rules_zoo_l2', 0), ('first_person_predators_prey', 0),
        ('cond_zoo', 0), ('cond_zoo', 1), ('phase_zoo', 0), ('phase_zoo', 1), ('phase_zoo_l1', 0),
        ('phase_zoo_l1', 1), ('match_to_sample_l3', 0), ('match_to_sample_l3', 1), ('match_to_sample_l4', 0),
        ('match_to_sample_l2', 0), ('predators_arena_l2', 0), ('predators_arena_l2', 1), ('predators_arena_l1', 0),
        ('predators_arena_l3', 0), ('bounce_box_contact_prediction', 0), ('bounce_box_contact_prediction_l1', 0),
        ('red_green_l1', 0), ('red_green', 0), ('red_green_l3', 0), ('lookahead_zoo', 0), ('lookahead_zoo', 1),
        ('lookahead_zoo_l1', 0), ('lookahead_zoo_l1', 1), ('tracing_zoo', 0), ('tracing_zoo', 1),
        ('tracing_zoo_l1', 0), ('tracing_zoo_l1', 1), ('combo_zoo', 0), ('combo_zoo', 1), ('actions_zoo', 0),
        ('actions_zoo', 1), ('actions_zoo_l1', 0), ('cleanup', 0), ('cleanup', 1), ('aa_zoo', 0), ('aa_zoo_l1', 0),
        ('aa_zoo_l2', 0), ('aa_zoo_l3', 0), ('aa_zoo_l4', 0), ('aa_zoo_l5', 0), ('callables_zoo', 0),
        ('callables_zoo', 1), ('callables_zoo_l1', 0), ('callables_zoo_l2', 0), ('callables_zoo_l3', 0),
        ('callables_zoo_l3', 1), ('maze_zoo', 0), ('maze_zoo', 1), ('maze_zoo_l1', 0), ('maze_zoo_l2', 0),
        ('maze_zoo_l2', 1), ('pacman', 0), ('pacman', 1), ('pacman_l1', 0), ('sampler_zoo', 0), ('sampler_zoo', 1),
        ('sampler_zoo_l1', 0), ('parallelogram_catch', 0), ('parallelogram_catch', 1), ('parallelogram_catch_l1', 0),
        ('parallelogram_catch_l1', 1), ('parallelogram_catch_l2', 0), ('multi_tracking_with_feature_l3', 0),
        ('multi_tracking_with_feature_l3', 1), ('multi_tracking_with_feature_l1', 0), ('dependent_zoo', 0),
        ('dependent_zoo', 1), ('sampler_zoo_l2', 0), ('sampler_zoo_l2', 1), ('sampler_zoo_l3', 0),
        ('sampler_zoo_l3', 1), ('functional_maze@128', 0), ('functional_maze@128', 1), ('colliding_predators_32', 1),
        ('colliding_predators_32', 2), ('falling_balls_64', 2)]
# recordings that start later in an episode (make_golden.py `__skip__`): call 0 is no reset
MID_EPISODE_RUNS = (('falling_balls_64', 1), ('falling_balls_64', 2))
# (Round 2 limited the free-running window of the piled-up falling_balls_64 recording to 4 calls.  The divergence came
#  from one thing: numpy evaluates np.dot / 1-D norms through OpenBLAS, whose ddot rounds the second product into the sum
#  with a fused multiply-add.  With npdot2 / npnorm restated that way the recording is reproduced free-running for all 64
#  calls with a worst error of 0.)
FREE_WINDOW = {}
# the programs BASELINE.json measures (__graft_entry__.SPEC_WORKLOADS: the ones a specialised step kernel is built for)
BASELINE_PROGRAMS = ('colliding_predators_32', 'falling_balls_64', 'functional_maze@128', 'chase_avoid_torus')

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_bp = ctypes.POINTER(ctypes.c_uint8)


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def build_host_model(source, name):
    """ctypes.CDLL of tests/_build/lib<name>.so: the host model `source` (a kernel header of csrc/ compiled with g++ and
    walked lane by lane, tests/csrc/*.cpp), rebuilt when the source, include/moog_engine.h or any header of csrc/ is newer."""
    build = os.path.join(REPO, 'tests', '_build')
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, 'lib%s.so' % name)
    deps = [source, os.path.join(REPO, 'include', 'moog_engine.h')] + glob.glob(os.path.join(REPO, 'moog.github.io_amd', 'csrc', '*.h'))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in deps):
        tmp = so + '.%d.tmp' % os.getpid()   # (xdist workers may build at the same time)
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared', '-Wall',
                               '-Wno-unused-function', source, '-o', tmp])
        os.replace(tmp, so)
    return ctypes.CDLL(so)


@functools.lru_cache(maxsize=None)
def oracle():
    """Builds (if needed) and loads the CPU oracle."""
    src = os.path.join(ORACLE_DIR, 'moog_oracle.c')
    hdr = os.path.join(REPO, 'include', 'moog_engine.h')
    if (not os.path.exists(ORACLE_SO) or
            os.path.getmtime(ORACLE_SO) < max(os.path.getmtime(src), os.path.getmtime(hdr))):
        subprocess.check_call(['make', '-C', ORACLE_DIR, '-B', 'libmoog_oracle.so'],
                              stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(ORACLE_SO)
    lib.oracle_program_sizeof.restype = ctypes.c_int64
    assert lib.oracle_program_sizeof() == ctypes.sizeof(_abi.Program)
    return lib


class OracleEnv(object):
    """Host-side state records + oracle entry points for one compiled program."""

    def __init__(self, compiled, n_envs=1, seed=0, env_index0=0):
        self.c = compiled
        self.P = compiled.program
        self.L = compiled.layout
        self.n = n_envs
        self.seed, self.env_index0 = seed, env_index0
        self.f64 = np.zeros((n_envs, self.L.f64_per_env), np.float64)
        self.i32 = np.zeros((n_envs, self.L.i32_per_env), np.int32)
        self.reward = np.zeros(n_envs)
        self.discount = np.zeros(n_envs)
        self.step_type = np.zeros(n_envs, np.int32)
        self.image = np.zeros((n_envs, self.P.render.height, self.P.render.width, 3), np.uint8)
        self.lib = oracle()
        # PILRenderer(color_to_rgb=<a callable>): Python, evaluated here per live sprite and handed to the oracle's renderer
        # per (env, slot) -- the oracle's counterpart of moog_engine_set_color_override
        self.color_fn = getattr(compiled, 'color_fn', None)

    def _color_override(self):
        from moog import environment
        S = self.L.S
        rgb = np.zeros((self.n, S), np.uint32)
        alive = (self.i32[:, self.L.o_flags:self.L.o_flags + S] & _abi.MOOG_F_ALIVE) != 0
        col = self.f64[:, self.L.o_color:self.L.o_color + 3 * S].reshape(self.n, S, 3)
        for i, s_ in zip(*np.nonzero(alive)):
            rgb[i, s_] = environment.BatchedEnvironment._call_color_fn(self.color_fn, col[i, s_])
        return rgb

    def _inj(self, u):
        if u is None:
            return None, 0
        u = np.ascontiguousarray(u, np.float64).reshape(self.n, -1)
        return u, u.shape[1]

    def reset(self, uniforms=None, mask=None, render=True):
        if self.color_fn is not None and render:   # (the colours exist once the state does: draw afterwards)
            self.reset(uniforms, mask, render=False)
            self.render()
            return
        u, nu = self._inj(uniforms)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.lib.oracle_reset(ctypes.byref(self.P), _ptr(self.f64, _dp), _ptr(self.i32, _ip),
                              self.n, _ptr(m, _bp), _ptr(u, _dp), nu,
                              ctypes.c_uint64(self.seed), ctypes.c_int64(self.env_index0),
                              _ptr(self.reward, _dp), _ptr(self.discount, _dp),
                              _ptr(self.step_type, _ip), _ptr(self.image, _bp) if render else None)

    def step(self, actions, uniforms=None, render=True):
        if self.color_fn is not None and render:
            self.step(actions, uniforms, render=False)
            self.render()
            return
        u, nu = self._inj(uniforms)
        # float32 actions (the reference's Joystick spec): the scaling is a float32 product
        self.lib.oracle_set_action_f32(1 if getattr(actions, 'dtype', None) == np.float32 else 0)
        if self.P.n_actions > 1:   # Composite: [n, n_actions, 2] (a Grid move in component 0)
            a = np.ascontiguousarray(actions, np.float64).reshape(self.n, 2 * self.P.n_actions)
            af, ai = a, None
        elif self.P.action.kind == _abi.MOOG_ACTION_GRID:
            a = np.ascontiguousarray(actions, np.int32).reshape(self.n)
            af, ai = None, a
        else:
            a = np.ascontiguousarray(actions, np.float64).reshape(self.n, 2)
            af, ai = a, None
        self.lib.oracle_step(ctypes.byref(self.P), _ptr(self.f64, _dp), _ptr(self.i32, _ip),
                             self.n, _ptr(af, _dp), _ptr(ai, _ip), _ptr(u, _dp), nu,
                             ctypes.c_uint64(self.seed), ctypes.c_int64(self.env_index0),
                             _ptr(self.reward, _dp), _ptr(self.discount, _dp),
                             _ptr(self.step_type, _ip), _ptr(self.image, _bp) if render else None)

    def physics(self, uniforms=None, substep=False):
        u, nu = self._inj(uniforms)
        fn = self.lib.oracle_substep if substep else self.lib.oracle_physics
        fn(ctypes.byref(self.P), _ptr(self.f64, _dp), _ptr(self.i32, _ip), self.n,
           _ptr(u, _dp), nu, ctypes.c_uint64(self.seed), ctypes.c_int64(self.env_index0))

    def render(self):
        rgb = None
        if self.color_fn is not None:
            rgb = self._color_override()
            self.lib.oracle_set_color_override(rgb.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(0))
        try:
            return self._render()
        finally:
            if rgb is not None:
                self.lib.oracle_set_color_override(None, ctypes.c_int64(0))

    def _render(self):
        self.lib.oracle_render(ctypes.byref(self.P), _ptr(self.f64, _dp), _ptr(self.i32, _ip),
                               self.n, _ptr(self.image, _bp))
        return self.image


@functools.lru_cache(maxsize=None)
def compiled(name):
    return _compiler.compile_config(layer_capacity=example_configs.capacity(name),
                                    **example_configs.load(name))


@functools.lru_cache(maxsize=None)
def fixture(name, seed=0):
    with np.load(os.path.join(GOLDEN, '%s_s%d.npz' % (name, seed))) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def collision_pairs():
    """tests/golden/collision_pairs.npz (make_golden.py make_collision_pairs): single pairs stepped once by the reference,
    with the branches it took.  Read only."""
    with np.load(os.path.join(GOLDEN, 'collision_pairs.npz')) as z:
        fx = {k: z[k] for k in z.files}
    for v in fx.values():
        v.setflags(write=False)
    return fx


def pair_rows(group):
    return np.flatnonzero(collision_pairs()['group'] == group)


def pair_config(group):
    """The drop-in config of a parameter group of the pair corpus: one placeholder sprite in each of the layers a and b (a
    30-vertex shape, so that every pair of the corpus fits the slots), the group's one Collision force between them."""
    import collections
    from moog import action_spaces, observers, physics as physics_lib, sprite, tasks
    el, sym, upd, u, depth = collision_pairs()['groups'][group]
    # shapes.SHAPES['circle'] is the 30-sided polygon: slot_vcap becomes 30, the corpus's VMAX (plant_pairs asserts the fit)
    s0 = sprite.Sprite(x=0.3, y=0.3, scale=0.1, shape='circle', c0=255)
    s1 = sprite.Sprite(x=0.7, y=0.7, scale=0.1, shape='circle', c1=255)
    f = physics_lib.Collision(elasticity=float(el), symmetric=bool(sym), update_angle_vel=bool(upd),
                              max_recursion_depth=int(depth))
    return dict(
        state_initializer=lambda: collections.OrderedDict([('a', [s0]), ('b', [s1]), ('agent', [])]),
        physics=physics_lib.Physics((f, 'a', 'b'), updates_per_env_step=int(u)),
        task=tasks.CompositeTask(),
        action_space=action_spaces.Grid(action_layers='agent'),
        observers={'image': observers.PILRenderer(image_size=(64, 64))})


def plant_pairs(c, f64, i32, before, rows):
    """Writes the before-records of pairs `rows` of the pair corpus `before` into the state records of a compiled
    pair_config program, pair rows[i] into env i: every field the step reads for a live sprite (records_from_fixture is the
    model).  Whatever else a reset left in the records (colours, opacity, counters) stays."""
    P, L = c.program, c.layout
    assert L.S == 2 and len(rows) <= len(f64)
    for env, r in enumerate(rows):
        f, q = f64[env], i32[env]
        for s in (0, 1):
            nv = int(before['nverts'][r, s])
            assert before['alive'][r, s] and nv <= P.slot_vcap[s]
            f[L.o_pos + 2 * s:L.o_pos + 2 * s + 2] = before['pos'][r, s]
            f[L.o_vel + 2 * s:L.o_vel + 2 * s + 2] = before['vel'][r, s]
            f[L.o_angle + s] = before['angle'][r, s]
            f[L.o_angvel + s] = before['angvel'][r, s]
            f[L.o_mass + s] = before['mass'][r, s]
            f[L.o_inertia + 2 * s:L.o_inertia + 2 * s + 2] = before['inertia'][r, s]
            f[L.o_maxr + s] = before['maxr'][r, s]
            o = L.o_verts + 2 * P.slot_voff[s]
            f[o:o + 2 * P.slot_vcap[s]] = 0
            f[o:o + 2 * nv] = before['verts'][r, s, :nv].ravel()
            fl = _abi.MOOG_F_ALIVE
            if before['sym_circle'][r, s]:
                fl |= _abi.MOOG_F_SYM_CIRCLE
            if before['vel_f32'][r, s]:
                fl |= _abi.MOOG_F_VEL_F32
            if before['angvel_f32'][r, s]:
                fl |= _abi.MOOG_F_ANGVEL_F32
            q[L.o_flags + s] = fl
            q[L.o_nverts + s] = nv
    return f64, i32


def pair_errors(c, f64, i32, fx, rows):
    """Compares pos / vel / angle / angvel of both sprites of env i with the recorded after-values of pair rows[i]:
    (worst |got - recorded| per pair [len(rows)], flags_ok [len(rows)]).  A NaN the reference produced (a symmetric or
    rotating collision with an infinite mass divides inf by inf) must be a NaN, anything else counts as an infinite error."""
    L = c.layout
    n = len(rows)
    f, q = f64[:n], i32[:n]
    got = dict(pos=f[:, L.o_pos:L.o_pos + 4].reshape(n, 2, 2), vel=f[:, L.o_vel:L.o_vel + 4].reshape(n, 2, 2),
               angle=f[:, L.o_angle:L.o_angle + 2], angvel=f[:, L.o_angvel:L.o_angvel + 2])
    worst = np.zeros(n)
    for key, g in got.items():
        ref = fx['after_' + key][rows]
        with np.errstate(invalid='ignore'):
            d = np.abs(g - ref)
        d = np.where(np.isnan(g) & np.isnan(ref), 0.0, d)
        d = np.where(g == ref, 0.0, d)   # (equal infinities)
        d = np.where(np.isnan(d), np.inf, d)
        worst = np.maximum(worst, d.reshape(n, -1).max(axis=1))
    fl = q[:, L.o_flags:L.o_flags + 2]
    flags_ok = (np.all(((fl & _abi.MOOG_F_VEL_F32) != 0) == (fx['after_vel_f32'][rows] != 0), axis=1) &
                np.all(((fl & _abi.MOOG_F_ANGVEL_F32) != 0) == (fx['after_angvel_f32'][rows] != 0), axis=1) &
                np.all((fl & _abi.MOOG_F_ALIVE) != 0, axis=1))
    return worst, flags_ok


PAIR_TOL = 1e-9   # the bar collisions_kat.npz is held to


def assert_pairs(c, f64, i32, fx, rows, who):
    """The assertion shared by the oracle test and the HIP test; names the pairs that miss, with their class bits."""
    worst, flags_ok = pair_errors(c, f64, i32, fx, rows)
    faults = i32[:len(rows), c.layout.o_fault]
    bad = np.flatnonzero((worst > PAIR_TOL) | ~flags_ok | (faults != 0))
    names = [str(x) for x in fx['classes']]
    report = ['pair %d (error %.3g, flags %s, fault %d): %s' % (
        rows[i], worst[i], 'ok' if flags_ok[i] else 'DIFFER', faults[i],
        ' '.join(nm for k, nm in enumerate(names) if (int(fx['cls'][rows[i]]) >> k) & 1)) for i in bad[:12]]
    print('%s: %d pairs, worst |%s - reference| %.3g' % (who, len(rows), who, float(worst.max())))
    assert len(bad) == 0, '%d of %d pairs differ from the reference:\n%s' % (len(bad), len(rows), '\n'.join(report))
    return float(worst.max())


# files named like a recording that hold one but have a test of their own (tests/test_views_gpu.py, tests/test_views.py: the
# several-observer recordings of tests/golden/make_golden_views.py) -- named one by one, so that no new file hides behind a pattern
RECORDINGS_WITH_OWN_TESTS = (('views_zoo_l0', 0), ('views_zoo_l1', 0), ('views_zoo_l2', 0))


def recordings_on_disk():
    """(name, seed) of every tests/golden/<name>_s<seed>.npz that holds a recording (key `step_type`)."""
    import re
    found = []
    for fn in sorted(os.listdir(GOLDEN)):
        m = re.match(r'(.+)_s(\d+)\.npz$', fn)
        if not m:
            continue
        with np.load(os.path.join(GOLDEN, fn)) as z:
            if 'step_type' in z.files:
                found.append((m.group(1), int(m.group(2))))
    return found


def ref_rules(c, n_ref):
    """(program rule, index of the config's rule object in the fixture's pre-order walk) for the rules that stand for a
    rule object of the config (a config-local rule may be lowered to several program rules, _compiler.rule_ref_index)."""
    ref = getattr(c, 'rule_ref_index', None) or list(range(c.program.n_rules))
    return [(r, k) for r, k in enumerate(ref) if 0 <= k < n_ref]


def portal_rule_mask(P):
    m = 0
    for r in range(P.n_rules):
        if P.rules[r].kind == _abi.MOOG_RULE_PORTAL:
            m |= 1 << r
    return m


def records_from_fixture(fx, t, c, f64=None, i32=None, env=0):
    """Writes the reference state of call `t` into state records (env row)."""
    P, L = c.program, c.layout
    S = L.S
    assert list(fx['layer_caps']) == [P.layer_nslots[i] for i in range(P.n_layers)], \
        'fixture slot table does not match the compiled program'
    if f64 is None:
        f64 = np.zeros((1, L.f64_per_env))
        i32 = np.zeros((1, L.i32_per_env), np.int32)
    f, q = f64[env], i32[env]
    f[:] = 0
    q[:] = 0
    nz = lambda a: np.nan_to_num(np.asarray(a, np.float64), nan=0.0, posinf=np.inf, neginf=-np.inf)
    f[L.o_pos:L.o_pos + 2 * S] = nz(fx['pos'][t]).ravel()
    f[L.o_vel:L.o_vel + 2 * S] = nz(fx['vel'][t]).ravel()
    f[L.o_angle:L.o_angle + S] = nz(fx['angle'][t])
    f[L.o_angvel:L.o_angvel + S] = nz(fx['angvel'][t])
    f[L.o_mass:L.o_mass + S] = nz(fx['mass'][t])
    f[L.o_color:L.o_color + 3 * S] = nz(fx['color'][t]).ravel()
    f[L.o_inertia:L.o_inertia + 2 * S] = nz(fx['inertia'][t]).ravel()
    f[L.o_maxr:L.o_maxr + S] = nz(fx['maxr'][t])
    am = np.asarray(fx['action_mem'][t], np.float64).reshape(-1)
    f[L.o_action:L.o_action + len(am)] = am
    tc = np.asarray(fx['task_counters'][t], np.float64).reshape(-1)
    for k in range(P.n_tasks):
        f[L.o_task + k] = tc[k] if k < len(tc) and not np.isnan(tc[k]) else np.inf
    # the fixture lists env.game_rules (top level); the program table is the pre-order forest
    rc = np.asarray(fx['rule_counters'][t], np.float64).reshape(-1)
    tops = [r for r in range(P.n_rules) if P.rules[r].parent < 0]
    for r in range(P.n_rules):
        f[L.o_rule + r] = np.inf
    for k, r in enumerate(tops):
        if k < len(rc) and not np.isnan(rc[k]):
            f[L.o_rule + r] = rc[k]
    if 'rule_counters_flat' in fx:   # newer fixtures: every rule of the pre-order forest
        flat = np.asarray(fx['rule_counters_flat'][t], np.float64).reshape(-1)
        for r, k in ref_rules(c, len(flat)):
            if not np.isnan(flat[k]):
                f[L.o_rule + r] = flat[k]
    if P.rule_state2:   # the duration a Phase drew when it was reset
        flat2 = np.asarray(fx['rule_counters2_flat'][t], np.float64).reshape(-1)
        for r in range(P.n_rules):
            f[L.o_rule2 + r] = 0.0
        for r, k in ref_rules(c, len(flat2)):
            f[L.o_rule2 + r] = 0.0 if np.isnan(flat2[k]) else flat2[k]
    for slot, key, cell, table in (getattr(c, 'dynamic_meta', None) or []):
        # what the initializer's look-ahead stored in a sprite's metadata: the engine keeps the exit the look-ahead took
        keys = [str(x) for x in np.asarray(fx['meta_keys'][t]).reshape(-1)]
        val = float(np.asarray(fx['meta_vals'][t])[slot, keys.index(key)])
        match = [ex for ex, v in table.items() if v == val or (np.isnan(v) and np.isnan(val))]
        assert match, ('metadata value the look-ahead cannot produce', key, val, table)
        f[L.o_hdraw + cell] = float(match[0])
    if getattr(c, 'pstate_slots', None):   # numbers the initializer keeps across episodes: never cleared by resets
        names = [str(x) for x in np.asarray(fx['init_state_names'][t]).reshape(-1)]
        vals = np.asarray(fx['init_state'][t], np.float64).reshape(-1)
        for name, ri in c.pstate_slots:
            f[L.o_rule + ri] = vals[names.index(name)]
            f[L.o_rule2 + ri] = 1.0
    if 'force_state' in fx:   # forces with state of their own (DeterministicMazeWalk's read position: a MOOG_RULE_STATE_SLOT)
        fs = np.asarray(fx['force_state'][t], np.float64).reshape(-1)
        for fi in range(min(P.n_forces, len(fs))):
            if P.forces[fi].kind == _abi.MOOG_FORCE_MAZE_WALK_DET:
                f[L.o_rule + P.forces[fi].symmetric] = fs[fi]
    pm = portal_rule_mask(P)
    for s in range(S):
        nv = int(fx['nverts'][t][s])
        assert nv <= P.slot_vcap[s]
        o = L.o_verts + 2 * P.slot_voff[s]
        f[o:o + 2 * nv] = fx['verts'][t][s, :nv].ravel()
        fl = 0
        if fx['alive'][t][s]:
            fl |= _abi.MOOG_F_ALIVE
        if fx['sym_circle'][t][s]:
            fl |= _abi.MOOG_F_SYM_CIRCLE
        if fx['vel_f32'][t][s]:
            fl |= _abi.MOOG_F_VEL_F32
        if fx['angvel_f32'][t][s]:
            fl |= _abi.MOOG_F_ANGVEL_F32
        q[L.o_flags + s] = fl
        q[L.o_nverts + s] = nv if fx['alive'][t][s] else 0
        q[L.o_opacity + s] = fx['opacity'][t][s]
        q[L.o_tele + s] = pm if fx['tele'][t][s] else 0
        if P.vel_alias:
            q[L.o_valias + s] = fx['vel_group'][t][s] if 'vel_group' in fx else 0
        if P.sprite_factors:
            f[L.o_scale + s] = nz(fx['scale'][t][s])
            f[L.o_aspect + s] = nz(fx['aspect'][t][s])
            q[L.o_fmask + s] = fx['fmask'][t][s]
    q[L.o_step_count] = fx['step_count'][t]
    q[L.o_reset_next] = fx['reset_next'][t]
    if P.maze.random:   # the episode's maze: what Maze.from_state reads off the recorded wall squares
        rows = maze_rows_from_fixture(fx, t, c)
        q[L.o_maze:L.o_maze + len(rows)] = rows
    return f64, i32


def maze_rows_from_fixture(fx, t, c):
    """Row bit masks (bit column = wall) of the maze whose wall squares call t of a recording holds."""
    P = c.program
    n = P.maze.size
    rows = np.zeros(_abi.MOOG_MAX_MAZE, np.int64)
    for oi in range(P.n_ops):
        if P.ops[oi].cell_sel != _abi.MOOG_CELL_WALL_RANK:
            continue
        s = P.ops[oi].slot0
        if not fx['alive'][t][s]:
            continue
        v = fx['verts'][t][s, :4]
        j, i = int(round(v[:, 0].min() * n)), int(round(v[:, 1].min() * n))
        rows[i] |= 1 << j
    return rows.astype(np.int32)


def state_diff(fx, t, c, f64, i32, env=0):
    """Max abs differences between the records and the reference state of call t.

    Returns dict(float=max abs error over live sprites' float state incl. vertices,
    ints_ok=bool for alive mask / nverts / counters / step bookkeeping, detail=str)."""
    P, L = c.program, c.layout
    S = L.S
    f, q = f64[env], i32[env]
    alive_ref = fx['alive'][t].astype(bool)
    alive = (q[L.o_flags:L.o_flags + S] & _abi.MOOG_F_ALIVE).astype(bool)
    detail = []
    ints_ok = True
    if not np.array_equal(alive, alive_ref):
        ints_ok = False
        detail.append('alive %s vs %s' % (alive.astype(int), alive_ref.astype(int)))
    err = {}
    live = alive_ref & alive

    def cmp(name, got, ref):
        got, ref = np.asarray(got, np.float64)[live], np.asarray(ref, np.float64)[live]
        if got.size == 0:
            err[name] = 0.0
            return
        with np.errstate(invalid='ignore'):
            d = np.abs(got - ref)
        d = np.where(np.isnan(got) & np.isnan(ref), 0.0, d)
        d = np.where(np.isinf(got) & (got == ref), 0.0, d)
        err[name] = float(np.max(d)) if not np.isnan(d).any() else np.inf

    cmp('pos', f[L.o_pos:L.o_pos + 2 * S].reshape(S, 2), fx['pos'][t])
    cmp('vel', f[L.o_vel:L.o_vel + 2 * S].reshape(S, 2), fx['vel'][t])
    cmp('angle', f[L.o_angle:L.o_angle + S], fx['angle'][t])
    cmp('angvel', f[L.o_angvel:L.o_angvel + S], fx['angvel'][t])
    cmp('mass', f[L.o_mass:L.o_mass + S], fx['mass'][t])
    cmp('color', f[L.o_color:L.o_color + 3 * S].reshape(S, 3), fx['color'][t])
    verr = 0.0
    for s in range(S):
        if not live[s]:
            continue
        nv = int(fx['nverts'][t][s])
        if int(q[L.o_nverts + s]) != nv:
            ints_ok = False
            detail.append('nverts[%d] %d vs %d' % (s, q[L.o_nverts + s], nv))
            continue
        o = L.o_verts + 2 * P.slot_voff[s]
        verr = max(verr, float(np.max(np.abs(f[o:o + 2 * nv] - fx['verts'][t][s, :nv].ravel()))))
        fl = int(q[L.o_flags + s])
        for bit, key in ((_abi.MOOG_F_SYM_CIRCLE, 'sym_circle'), (_abi.MOOG_F_VEL_F32, 'vel_f32'),
                         (_abi.MOOG_F_ANGVEL_F32, 'angvel_f32')):
            if bool(fl & bit) != bool(fx[key][t][s]):
                ints_ok = False
                detail.append('flag %s slot %d' % (key, s))
        if bool(q[L.o_tele + s]) != bool(fx['tele'][t][s]):
            ints_ok = False
            detail.append('tele slot %d' % s)
        if int(q[L.o_opacity + s]) != int(fx['opacity'][t][s]):
            ints_ok = False
            detail.append('opacity slot %d' % s)
    err['verts'] = verr
    if P.sprite_factors and 'scale' in fx:
        cmp('scale', f[L.o_scale:L.o_scale + S], fx['scale'][t])
        cmp('aspect', f[L.o_aspect:L.o_aspect + S], fx['aspect'][t])
        relevant = sum(1 << b for b in (_abi.MOOG_FAC_SCALE, _abi.MOOG_FAC_ASPECT, _abi.MOOG_FAC_C0,
                                        _abi.MOOG_FAC_C1, _abi.MOOG_FAC_C2, _abi.MOOG_FAC_MASS))
        for s in range(S):
            if live[s] and (int(q[L.o_fmask + s]) ^ int(fx['fmask'][t][s])) & relevant:
                ints_ok = False
                detail.append('float32 factor mask slot %d: %x vs %x' % (s, q[L.o_fmask + s], fx['fmask'][t][s]))
    if P.vel_alias and 'vel_group' in fx:
        # sprites sharing one velocity ndarray: same partition (the group ids are arbitrary)
        def canon(g):
            g = np.where(live, np.asarray(g), 0)
            return [0 if g[s] == 0 else 1 + int(np.flatnonzero(g == g[s])[0]) for s in range(S)]
        if canon(q[L.o_valias:L.o_valias + S]) != canon(fx['vel_group'][t]):
            ints_ok = False
            detail.append('shared-velocity groups %s vs %s' % (
                canon(q[L.o_valias:L.o_valias + S]), canon(fx['vel_group'][t])))
    if int(q[L.o_step_count]) != int(fx['step_count'][t]) or \
            int(q[L.o_reset_next]) != int(fx['reset_next'][t]):
        ints_ok = False
        detail.append('step_count/reset_next %d/%d vs %d/%d' % (
            q[L.o_step_count], q[L.o_reset_next], fx['step_count'][t], fx['reset_next'][t]))
    if 'rule_counters_flat' in fx:   # every rule of the pre-order forest (NaN: the reference rule keeps no number)
        flat = np.asarray(fx['rule_counters_flat'][t], np.float64).reshape(-1)
        for r, k in ref_rules(c, len(flat)):
            if not np.isnan(flat[k]) and f[L.o_rule + r] != flat[k]:
                ints_ok = False
                detail.append('rule %d state: %r vs %r' % (r, f[L.o_rule + r], flat[k]))
    if P.rule_state2:
        flat2 = np.asarray(fx['rule_counters2_flat'][t], np.float64).reshape(-1)
        for r, k in ref_rules(c, len(flat2)):
            if P.rules[r].op == 1 and P.rules[r].kind == _abi.MOOG_RULE_PHASE and f[L.o_rule2 + r] != flat2[k]:
                ints_ok = False
                detail.append('phase %d duration: %r vs %r' % (r, f[L.o_rule2 + r], flat2[k]))
    if getattr(c, 'pstate_slots', None):
        names = [str(x) for x in np.asarray(fx['init_state_names'][t]).reshape(-1)]
        vals = np.asarray(fx['init_state'][t], np.float64).reshape(-1)
        for name, ri in c.pstate_slots:
            if f[L.o_rule + ri] != vals[names.index(name)]:
                ints_ok = False
                detail.append('initializer state %s: %r vs %r' % (name, f[L.o_rule + ri], vals[names.index(name)]))
    if 'force_state' in fx:
        fs = np.asarray(fx['force_state'][t], np.float64).reshape(-1)
        for fi in range(min(P.n_forces, len(fs))):
            if P.forces[fi].kind == _abi.MOOG_FORCE_MAZE_WALK_DET and f[L.o_rule + P.forces[fi].symmetric] != fs[fi]:
                ints_ok = False
                detail.append('force %d state: %r vs %r' % (fi, f[L.o_rule + P.forces[fi].symmetric], fs[fi]))
    if P.maze.random:
        rows = maze_rows_from_fixture(fx, t, c)
        if not np.array_equal(q[L.o_maze:L.o_maze + len(rows)], rows):
            ints_ok = False
            detail.append('maze rows %s vs %s' % (list(q[L.o_maze:L.o_maze + P.maze.size]), list(rows[:P.maze.size])))
    ref_am = np.asarray(fx['action_mem'][t], np.float64).reshape(-1)
    am = float(np.max(np.abs(f[L.o_action:L.o_action + len(ref_am)] - ref_am)))
    err['action_mem'] = am
    tc = np.asarray(fx['task_counters'][t], np.float64).reshape(-1)
    for k in range(min(P.n_tasks, len(tc))):
        if not np.isnan(tc[k]) and f[L.o_task + k] != tc[k]:
            ints_ok = False
            detail.append('task counter %d: %r vs %r' % (k, f[L.o_task + k], tc[k]))
    rc = np.asarray(fx['rule_counters'][t], np.float64).reshape(-1)
    tops = [r for r in range(P.n_rules) if P.rules[r].parent < 0]
    for k, r in enumerate(tops[:len(rc)]):
        if not np.isnan(rc[k]) and f[L.o_rule + r] != rc[k]:
            ints_ok = False
            detail.append('rule counter %d: %r vs %r' % (k, f[L.o_rule + r], rc[k]))
    if 'rule_counters_flat' in fx:
        flat = np.asarray(fx['rule_counters_flat'][t], np.float64).reshape(-1)
        for r, k in ref_rules(c, len(flat)):
            if not np.isnan(flat[k]) and f[L.o_rule + r] != flat[k]:
                ints_ok = False
                detail.append('rule state %d: %r vs %r' % (r, f[L.o_rule + r], flat[k]))
    return dict(float=max(err.values()), err=err, ints_ok=ints_ok, detail='; '.join(detail))


def action_of(fx, t):
    """The action of recorded call t, in the dtype the reference was handed (float32 for recordings made with the
    Joystick spec's own dtype, tests/golden/make_golden.py `__action_f32__`)."""
    a = np.asarray(fx['action'][t])
    if 'action_f32' in fx and int(fx['action_f32']):
        a = a.astype(np.float32)
    return a


def uniforms_of(fx, t):
    n = int(fx['n_uniforms'][t])
    return np.ascontiguousarray(fx['uniforms'][t, :max(n, 1)]).copy() if n else None


def same_or_nan(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))
