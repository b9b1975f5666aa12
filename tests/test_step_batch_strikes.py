"""The strikes collision_same_layer takes from a narrow batch (csrc/moog_device.h): every group of a batch that the edge tests
rejected has its own bit struck, and the bit of its mirror image too when no pair of parallel edges was among those tested.
A strike only removes a visit that would change nothing, so results must not move by a bit.

CPU part (oracle only): the cases do hold what the strikes touch -- near-miss candidates in every env, pairs that START to
overlap between their two visits of a sub-step (where a stale strike would show), and near misses with parallel facing edges
(where the mirror must not be struck).
GPU part: strikes on against strikes off (debug word 512 | 1024) bit for bit on the generic kernel, and the specialised and
generic kernels free-running against the oracle at the bar of tests/test_step_contact_path.py (integers exact, floats
within 1e-5, no fault word).  One oracle trajectory per case and test session, shared by the tests and left unchanged; the
pile-up of falling_balls_64 is that file's case and trajectory."""
import collections
import ctypes
import functools

import numpy as np
import pytest

import helpers
import test_step_contact_path as contact_path
from helpers import compiled

N = contact_path.N
TOL = contact_path.TOL
gpu = pytest.mark.gpu

# ---- the planted scene: a row of identical rectangles at 30 degrees, end to end along their long axis ------------------
ROW_N = 10
ROW_ANGLE = np.pi / 6          # no multiple of 45 degrees: the facing edges lie along none of the 8-DOP's axes
ROW_LEN, ROW_H = 0.07, 0.035   # length (along the row) and height of a rectangle
ROW_GAP = 0.01 * ROW_LEN       # between neighbours: the 8-DOPs overlap, the polygons do not
ROW_CALLS = 20


def row_config():
    """ROW_N rectangles in one layer with a symmetric Collision of the layer with itself; nothing else moves them.  All
    angular velocities are zero and contacts leave them alone (update_angle_vel=False): facing edges stay parallel."""
    from moog import action_spaces, observers, physics as physics_lib, sprite, tasks
    u = np.array([np.cos(ROW_ANGLE), np.sin(ROW_ANGLE)])
    rect = np.array([[-1., -1.], [1., -1.], [1., 1.], [-1., 1.]]) * [ROW_LEN / 2, ROW_H / 2]
    row = []
    for k in range(ROW_N):
        p = 0.5 + (k - (ROW_N - 1) / 2) * (ROW_LEN + ROW_GAP) * u
        row.append(sprite.Sprite(x=float(p[0]), y=float(p[1]), shape=rect, angle=ROW_ANGLE, scale=1., c0=255))
    f = physics_lib.Collision(elasticity=1., symmetric=True, update_angle_vel=False)
    return dict(
        state_initializer=lambda: collections.OrderedDict([('row', row), ('agent', [])]),
        physics=physics_lib.Physics((f, 'row', 'row'), updates_per_env_step=10),
        task=tasks.CompositeTask(),
        action_space=action_spaces.Grid(action_layers='agent'),
        observers={'image': observers.PILRenderer(image_size=(64, 64))})


@functools.lru_cache(maxsize=None)
def row_compiled():
    from moog import _compiler
    return _compiler.compile_config(**row_config())


def plant_row_velocities(c, f64):
    """Env i, rectangle k: (-1)^k (1 + i / 8) 4e-4 along the row, so that neighbours close their gap within two calls and
    the row goes on exchanging velocities face to face; the odd envs drift across the row as well (edges slide along each
    other).  Env 0 keeps every rectangle at rest: nothing but near misses."""
    L = c.layout
    u = np.array([np.cos(ROW_ANGLE), np.sin(ROW_ANGLE)])
    w = np.array([-u[1], u[0]])
    for i in range(1, len(f64)):
        for k in range(ROW_N):
            v = (-1) ** k * (1 + i / 8) * 4e-4 * u + (i % 2) * (k % 3 - 1) * 1e-4 * w
            f64[i, L.o_vel + 2 * k:L.o_vel + 2 * k + 2] = v
    return f64


@functools.lru_cache(maxsize=None)
def row_oracle_run():
    """The oracle's trajectory of the planted scene, shaped like contact_path.oracle_run's (read only)."""
    c = row_compiled()
    o = helpers.OracleEnv(c, n_envs=N, seed=2)
    o.reset(render=False)
    plant_row_velocities(c, o.f64)
    f0, q0 = o.f64.copy(), o.i32.copy()
    acts, F, Q, R, ST = [], [], [], [], []
    for _ in range(ROW_CALLS):
        a = np.full(N, 4, np.int32)   # (no agent: the action moves nothing)
        o.step(a, render=False)
        acts.append(a); F.append(o.f64.copy()); Q.append(o.i32.copy()); R.append(o.reward.copy()); ST.append(o.step_type.copy())
    out = (f0, q0, acts, F, Q, R, ST)
    for x in (f0, q0) + tuple(acts) + tuple(F) + tuple(Q) + tuple(R) + tuple(ST):
        x.setflags(write=False)
    return out


PRED_SEED, PRED_CALLS = 6, 40   # (chosen on the CPU among seeds 1 - 12 for test_pairs_start_to_overlap_between_their_two_visits: 30 events)


@functools.lru_cache(maxsize=None)
def predators_oracle_run():
    """colliding_predators_32 from the start of tests/test_step_contact_path.py -- a seeded reset, env i put 6 + i steps
    before the 200-step timeout, so that every env auto-resets inside the 40 calls, each at a call of its own -- with
    another seed; shaped like contact_path.oracle_run's trajectory (read only)."""
    c = compiled('colliding_predators_32')
    o = helpers.OracleEnv(c, n_envs=N, seed=PRED_SEED)
    o.reset(render=False)
    o.i32[:, c.layout.o_step_count] = c.program.timeout_steps - 6 - np.arange(N)
    f0, q0 = o.f64.copy(), o.i32.copy()
    rs = np.random.RandomState(3)
    acts, F, Q, R, ST = [], [], [], [], []
    for _ in range(PRED_CALLS):
        a = rs.uniform(-1, 1, size=(N, 2))
        o.step(a, render=False)
        acts.append(a); F.append(o.f64.copy()); Q.append(o.i32.copy()); R.append(o.reward.copy()); ST.append(o.step_type.copy())
    assert sum(int(np.sum(st == 0)) for st in ST) == N   # (the auto-resets)
    out = (f0, q0, acts, F, Q, R, ST)
    for x in (f0, q0) + tuple(acts) + tuple(F) + tuple(Q) + tuple(R) + tuple(ST):
        x.setflags(write=False)
    return out


SEEDS = {'colliding_predators_32': PRED_SEED, 'row': 2, 'falling_balls_64': 5}


def case(name):
    """(compiled program, its oracle trajectory, the slots [s0, s1) of the layer collided with itself)."""
    if name == 'row':
        c = row_compiled()
        return c, row_oracle_run(), (c.program.layer_slot0[0], c.program.layer_slot0[0] + c.program.layer_nslots[0])
    c = compiled(name)
    run = predators_oracle_run() if name == 'colliding_predators_32' else contact_path.oracle_run(name)
    return c, run, (c.program.layer_slot0[1], c.program.layer_slot0[1] + c.program.layer_nslots[1])


# ---- numpy restatements -----------------------------------------------------------------------------------------------
def polygons(c, f, q, s0, s1):
    """[(slot, vertices [n, 2], position [2], bounding radius)] of the live sprites of slots [s0, s1) of one env's record."""
    P, L = c.program, c.layout
    out = []
    for s in range(s0, s1):
        if q[L.o_flags + s] & helpers._abi.MOOG_F_ALIVE:
            n, o = int(q[L.o_nverts + s]), L.o_verts + 2 * P.slot_voff[s]
            out.append((s, f[o:o + 2 * n].reshape(n, 2), f[L.o_pos + 2 * s:L.o_pos + 2 * s + 2], f[L.o_maxr + s]))
    return out


def dop8(v):
    """Exact 8-DOP: (minima, maxima) of x, y, x + y, x - y."""
    a = np.stack([v[:, 0], v[:, 1], v[:, 0] + v[:, 1], v[:, 0] - v[:, 1]])
    return a.min(1), a.max(1)


def candidates(polys):
    """The unordered pairs (a, b), a before b, whose bounding circles (sprite.py:464-466) and exact 8-DOPs are not apart."""
    dops = [dop8(p[1]) for p in polys]
    out = []
    for i in range(len(polys)):
        for j in range(i + 1, len(polys)):
            if np.linalg.norm(polys[i][2] - polys[j][2]) > polys[i][3] + polys[j][3]:
                continue
            (la, ha), (lb, hb) = dops[i], dops[j]
            if np.any(la > hb) or np.any(lb > ha):
                continue
            out.append((i, j))
    return out


def isclose(a, b):
    return abs(a - b) <= max(1e-10 * max(abs(a), abs(b)), 1e-13)


def segments_intersect_kind(x1, y1, x2, y2, x3, y3, x4, y4):
    """csrc/moog_device.h segments_intersect_kind (matplotlib's segments_intersect with the parallel branch told apart):
    0 no intersection, not parallel; 1 collinear and overlapping; 2 a crossing; 4 parallel, no intersection."""
    den = ((y4 - y3) * (x2 - x1)) - ((x4 - x3) * (y2 - y1))
    if isclose(den, 0.0):
        t_area = (x2 * y3 - x3 * y2) - x1 * (y3 - y2) + y1 * (x3 - x2)
        if isclose(t_area, 0.0):
            if x1 == x2 and x2 == x3:
                return 1 if ((min(y1, y2) <= min(y3, y4) <= max(y1, y2)) or (min(y3, y4) <= min(y1, y2) <= max(y3, y4))) else 4
            return 1 if ((min(x1, x2) <= min(x3, x4) <= max(x1, x2)) or (min(x3, x4) <= min(x1, x2) <= max(x3, x4))) else 4
        return 4
    n1 = ((x4 - x3) * (y1 - y3)) - ((y4 - y3) * (x1 - x3))
    n2 = ((x2 - x1) * (y1 - y3)) - ((y2 - y1) * (x1 - x3))
    u1, u2 = n1 / den, n2 / den
    ok = lambda u: (u > 0.0 or isclose(u, 0.0)) and (u < 1.0 or isclose(u, 1.0))
    return 2 if ok(u1) and ok(u2) else 0


BB_MARGIN = 1e-5   # csrc/moog_device.h: edges further apart than this along an axis are never tested


def edge_kinds(va, vb):
    """The answers of segments_intersect_kind over the edge pairs of two polygons that the engine's culls leave (an edge
    reaching the other polygon's 8-DOP along all four axes; the two edges' boxes within BB_MARGIN of each other)."""
    def reaching(v, lo, hi):
        keep = []
        for k in range(len(v)):
            e = np.stack([v[k], v[(k + 1) % len(v)]])
            lo_e, hi_e = dop8(e)
            if not (np.any(lo_e > hi + BB_MARGIN) or np.any(hi_e < lo - BB_MARGIN)):
                keep.append(e)
        return keep
    kinds = []
    for ea in reaching(va, *dop8(vb)):
        for eb in reaching(vb, *dop8(va)):
            if np.any(ea.min(0) > eb.max(0) + BB_MARGIN) or np.any(eb.min(0) > ea.max(0) + BB_MARGIN):
                continue
            kinds.append(segments_intersect_kind(*ea[0], *ea[1], *eb[0], *eb[1]))
    return kinds


@functools.lru_cache(maxsize=None)
def substep_survey(name):
    """Every call of a case's trajectory again, from the oracle's own record before the call, one sub-step at a time with
    the oracle's search log on (the sub-steps run one env after the other, which the log needs).  Per env: ordered
    same-layer candidates summed over the sub-steps, sub-steps, the searches of a pair (j, i), j > i, of the layer
    whose mirror image (i, j) was not searched earlier in the same sub-step, and the searches that found a contact."""
    c, (f0, q0, acts, F, Q, R, ST), (s0, s1) = case(name)
    K = c.program.updates_per_env_step
    lib = helpers.oracle()
    o = helpers.OracleEnv(c, n_envs=N, seed=SEEDS[name])
    buf = np.zeros(1 << 20, np.int32)
    cands, late, contacts = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64)
    for t in range(len(acts)):
        o.f64[:], o.i32[:] = (f0, q0) if t == 0 else (F[t - 1], Q[t - 1])
        for k in range(K):
            for i in range(N):
                cands[i] += 2 * len(candidates(polygons(c, o.f64[i], o.i32[i], s0, s1)))
            lib.oracle_contact_log(buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(buf))
            o.physics(substep=True)
            m = lib.oracle_contact_log_count()
            lib.oracle_contact_log(None, 0)
            assert m < len(buf) - 2
            env, seen, deep = None, None, False
            for a, b in buf[:m].reshape(-1, 2):
                if a == -1:
                    env, seen = int(b) - o.env_index0, set()
                elif a == -2:   # the next outcome is a search at depth > 0 of Collision.step's recursion: no visit of the cursor
                    deep = True
                elif -5 <= a <= -3:   # the outcome of a search (CV_NONE, CV_OK, CV_FUTURE) of pair (b & 255, b >> 8 & 255)
                    if deep:
                        deep = False
                        contacts[env] += a == -4
                        continue
                    j, i = int(b) & 255, (int(b) >> 8) & 255
                    if s0 <= i < j < s1 and (i, j) not in seen and (j, i) not in seen:
                        late[env] += 1
                    seen.add((j, i))
                    contacts[env] += a == -4
    return cands, K * len(acts), late, contacts


# ---- CPU preconditions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['colliding_predators_32', 'row'])
def test_near_miss_pairs_are_present(name):
    """(a) Every env of the case averages at least two ordered same-layer broad-phase candidates per sub-step (bounding
    circles and exact 8-DOPs not apart) -- what the narrow batches are made of."""
    cands, substeps, _, _ = substep_survey(name)
    per = cands / substeps
    print('%s: ordered same-layer candidates per env and sub-step: min %.2f mean %.2f max %.2f' % (name, per.min(), per.mean(), per.max()))
    assert np.all(per >= 2), per


def test_pairs_start_to_overlap_between_their_two_visits():
    """(b) colliding_predators_32 over its 40 calls: searches of a pair (j, i), j > i, whose mirror image (i, j) -- visited
    earlier in the same sub-step -- was not searched: the pair came to overlap in between, through a contact of one of its
    sprites with a third.  A strike that outlived such a contact would take the search away and the run would leave the
    oracle's.  At least 20 over the case."""
    _, _, late, _ = substep_survey('colliding_predators_32')
    print('searches of (j, i) without an earlier search of (i, j) in the sub-step: %d (per env %s)' % (late.sum(), late.tolist()))
    assert late.sum() >= 20


def test_row_near_misses_have_parallel_facing_edges():
    """(c) The planted row at its start: at least 8 candidate pairs whose tested edge pairs include a parallel one without an
    intersection (answer 4: the mirror image must not be struck on this batch's word) and none that intersects (1 or 2)."""
    c, (f0, q0, acts, F, Q, R, ST), (s0, s1) = case('row')
    polys = polygons(c, f0[0], q0[0], s0, s1)
    assert len(polys) == ROW_N and all(len(p[1]) == 4 for p in polys)
    n4 = 0
    for i, j in candidates(polys):
        kinds = edge_kinds(polys[i][1], polys[j][1])
        assert 1 not in kinds and 2 not in kinds, (i, j, kinds)
        n4 += 4 in kinds
    print('row: %d candidate pairs with a parallel facing edge pair and no intersection' % n4)
    assert n4 >= 8


def test_row_holds_contacts():
    """The planted row is no scene of near misses alone: in every env but the one at rest the five pairs (0, 1), (2, 3), ...
    start 7e-4 apart and close at 9e-4 per call or faster, so each resolves a contact (and the invalidation after it runs);
    the env at rest resolves none."""
    contacts = substep_survey('row')[3]
    print('row: searches that found a contact, per env', contacts.tolist())
    assert contacts[0] == 0 and np.all(contacts[1:] >= 5)


# ---- GPU --------------------------------------------------------------------------------------------------------------
def make_env(name):
    seed = SEEDS[name]
    from moog import environment
    from moog_demos import example_configs
    if name == 'row':
        return environment.BatchedEnvironment(num_envs=N, seed=seed, **row_config())
    return environment.BatchedEnvironment(num_envs=N, seed=seed, layer_capacity=example_configs.capacity(name), **example_configs.load(name))


@gpu
@pytest.mark.parametrize('name', ['colliding_predators_32', 'row'])
def test_strikes_on_equal_strikes_off(name, monkeypatch):
    """The generic kernel with every strike (debug word 0) and without the mirrored-pair and the batch strikes (512 | 1024)
    from the same records with the same actions: state records, rewards and step types bit-identical after every call."""
    import torch
    monkeypatch.setenv('MOOG_STEP_SPEC', '0')
    c, (f0, q0, acts, F, Q, R, ST), _ = case(name)
    envs = []
    for dbg in (0, 512 | 1024):
        env = make_env(name)
        assert env.step_kernel() == 'generic', env.step_kernel()
        env.reset()
        env.state_f64.copy_(torch.from_numpy(np.array(f0)))
        env.state_i32.copy_(torch.from_numpy(np.array(q0)))
        env.check_faults = False
        env.set_debug(dbg, 0)
        envs.append(env)
    for t, a in enumerate(acts):
        outs = [env.step(torch.from_numpy(np.array(a)).to(env.device)) for env in envs]
        torch.cuda.synchronize()
        bits = lambda x: x.cpu().numpy().view(np.int64)
        assert np.array_equal(bits(envs[0].state_f64), bits(envs[1].state_f64)), 'float records differ at call %d' % t
        assert np.array_equal(envs[0].state_i32.cpu().numpy(), envs[1].state_i32.cpu().numpy()), 'integer records differ at call %d' % t
        assert np.array_equal(bits(outs[0].reward), bits(outs[1].reward)), 'rewards differ at call %d' % t
        assert np.array_equal(outs[0].step_type.cpu().numpy(), outs[1].step_type.cpu().numpy()), 'step types differ at call %d' % t
        assert not np.any(envs[0].state_i32.cpu().numpy()[:, c.layout.o_fault]), t
    for env in envs:
        env.close()


def run_against_oracle(name, kernel, monkeypatch, spec_dir=None):
    """contact_path.run_case for the cases of this file: free-running, never re-synchronised.  `spec_dir`: where to build the
    program's specialised step kernel first (a program the build makes none for)."""
    import torch
    c, (f0, q0, acts, F, Q, R, ST), _ = case(name)
    if kernel == 'generic':
        monkeypatch.setenv('MOOG_STEP_SPEC', '0')
    else:   # the specialised step kernels the build made (lib/spec), or the one built here
        monkeypatch.delenv('MOOG_STEP_SPEC', raising=False)
        monkeypatch.delenv('MOOG_SPEC_DIR', raising=False)
        if spec_dir is not None:
            from moog import _spec
            monkeypatch.setenv('MOOG_SPEC_DIR', str(spec_dir))
            _spec.build(c.program)
    env = make_env(name)
    assert env.step_kernel() == kernel, env.step_kernel()   # (the claim is about that binary)
    env.reset()
    env.state_f64.copy_(torch.from_numpy(np.array(f0)))
    env.state_i32.copy_(torch.from_numpy(np.array(q0)))
    env.check_faults = False
    worst = 0.0
    for t, a in enumerate(acts):
        out = env.step(torch.from_numpy(np.array(a)).to(env.device))
        torch.cuda.synchronize()
        f, q = env.state_f64.cpu().numpy(), env.state_i32.cpu().numpy()
        assert np.array_equal(q, Q[t]), 'integer records differ from the oracle at call %d' % t
        with np.errstate(invalid='ignore'):
            err = np.abs(f - F[t])
        err = np.where(np.isnan(f) & np.isnan(F[t]), 0, err)
        err = np.where(f == F[t], 0, err)
        worst = max(worst, float(np.max(err)))
        assert worst <= TOL, (t, worst)
        assert np.array_equal(out.step_type.cpu().numpy(), ST[t]), t
        assert helpers.same_or_nan(out.reward.cpu().numpy(), R[t]), t
        assert not np.any(q[:, c.layout.o_fault]), t
    env.close()
    print('%s on the %s kernel: %d calls, worst |state - oracle| %.3g' % (name, kernel, len(acts), worst))


@gpu
@pytest.mark.parametrize('kernel', contact_path.KERNELS)
def test_colliding_predators_32_against_the_oracle(kernel, monkeypatch):
    """The headline program over 40 calls in which every env auto-resets once."""
    run_against_oracle('colliding_predators_32', kernel, monkeypatch)


@gpu
@pytest.mark.parametrize('kernel', contact_path.KERNELS)
def test_falling_balls_64_pile_up_against_the_oracle(kernel, monkeypatch):
    """The recorded pile-up of tests/test_step_contact_path.py, the first 20 of its calls: dense rows, 30-gons that take the
    ordinary path."""
    c, (f0, q0, acts, F, Q, R, ST), _ = case('falling_balls_64')
    monkeypatch.setattr(contact_path, 'oracle_run', lambda name: (f0, q0, acts[:20], F[:20], Q[:20], R[:20], ST[:20]))
    contact_path.run_case('falling_balls_64', kernel, monkeypatch)


@gpu
@pytest.mark.parametrize('kernel', contact_path.KERNELS)
def test_row_against_the_oracle(kernel, monkeypatch, tmp_path):
    """The planted row over 20 calls.  The build makes no specialised kernel for this program, so the case compiles one of
    its own (moog/_spec.py, as tests/test_gpu_parity.py::test_specialised_step_kernel_is_result_neutral does): in a specialised
    kernel the strikes cannot be switched off, and this is the scene whose batches see parallel edges."""
    run_against_oracle('row', kernel, monkeypatch, spec_dir=tmp_path)
