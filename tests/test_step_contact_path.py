"""The contact path of the step kernel (collision_same_layer's candidate cursor, the re-test after a contact, the mirrored-pair
strikes, contacts that change angular velocities) free-running against the CPU oracle, on the program-specialised and on the
generic step kernels.  Needs an MI355X.

Every case steps 16 envs and the oracle from the same records with the same actions, WITHOUT re-synchronising them: integer
records must stay identical, float records within the free-running bar of tests/test_gpu_parity.py (TOL = 1e-5: the device's
libm differs from the host's by an ulp here and there, and a chaotic system carries that along), rewards and step types
exact.  Each case also asserts, from the oracle's own trajectory, that contacts did happen -- x velocities (and angular
velocities) of the colliding layer only ever change in a contact in these programs -- so a contact-free run cannot pass.
The seeds were chosen on the CPU with the oracle alone (the counts are in each case's docstring)."""
import functools

import numpy as np
import pytest

import helpers
from helpers import compiled, fixture, records_from_fixture

pytestmark = pytest.mark.gpu
TOL = 1e-5
N = 16
KERNELS = ['specialised', 'generic']


def _start_colliding_predators_32(c):
    """A seeded reset (seed 5); env i is then put 6 + i steps before the 200-step timeout, so that every env times out and
    auto-resets inside the 40 calls, each at a call of its own."""
    o = helpers.OracleEnv(c, n_envs=N, seed=5)
    o.reset(render=False)
    o.i32[:, c.layout.o_step_count] = c.program.timeout_steps - 6 - np.arange(N)
    return o


def _start_falling_balls_64(c):
    """The recorded pile-up (tests/golden/falling_balls_64_s1.npz, which starts late in an episode): env i starts from the
    recorded state of call 2 i, so the 16 envs are 16 different piles."""
    fx = fixture('falling_balls_64', 1)
    o = helpers.OracleEnv(c, n_envs=N, seed=5)
    for i in range(N):
        records_from_fixture(fx, 2 * i, c, o.f64, o.i32, env=i)
    return o


def _start_colliding_predators(c):
    """A seeded reset (seed 11) of colliding_predators: five large predators with float32 velocities and float32 non-zero
    angular velocities in a small arena, update_angle_vel=True on both of their collisions."""
    o = helpers.OracleEnv(c, n_envs=N, seed=11)
    o.reset(render=False)
    return o


#        name                     start                           calls
CASES = {'colliding_predators_32': (_start_colliding_predators_32, 40),
         'falling_balls_64': (_start_falling_balls_64, 30),
         'colliding_predators': (_start_colliding_predators, 40)}


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """The oracle's trajectory of a case, computed once and shared by the kernels it is held against (read only):
    (start f64, start i32, actions [T], f64 [T], i32 [T], reward [T], step_type [T])."""
    start, T = CASES[name]
    c = compiled(name)
    o = start(c)
    f0, q0 = o.f64.copy(), o.i32.copy()
    rs = np.random.RandomState(3)
    grid = c.program.action.kind == helpers._abi.MOOG_ACTION_GRID
    acts, F, Q, R, ST = [], [], [], [], []
    for _ in range(T):
        a = rs.randint(0, 5, size=N).astype(np.int32) if grid else rs.uniform(-1, 1, size=(N, 2))
        o.step(a, render=False)
        acts.append(a); F.append(o.f64.copy()); Q.append(o.i32.copy()); R.append(o.reward.copy()); ST.append(o.step_type.copy())
    out = (f0, q0, acts, F, Q, R, ST)
    for x in (f0, q0) + tuple(acts) + tuple(F) + tuple(Q) + tuple(R) + tuple(ST):
        x.setflags(write=False)
    return out


def contact_counts(name):
    """From the oracle's trajectory: (sprite-calls of the colliding layer -- layer 1: predators / balls -- whose x velocity
    changed, ... whose angular velocity changed, auto-resets).  Nothing but a contact changes either in these programs
    (the predators feel no other force; gravity acts along y only); calls that reset an env are left out."""
    c = compiled(name)
    P, L = c.program, c.layout
    f0, q0, acts, F, Q, R, ST = oracle_run(name)
    s0, ns = P.layer_slot0[1], P.layer_nslots[1]
    vx = lambda f: f[:, L.o_vel + 2 * s0:L.o_vel + 2 * (s0 + ns):2]
    w = lambda f: f[:, L.o_angvel + s0:L.o_angvel + s0 + ns]
    nv = nw = resets = 0
    prev = f0
    for f, st in zip(F, ST):
        live = (st != 0)[:, None]   # (step type 0 = FIRST: the env was reset in this call)
        nv += int(np.sum((vx(f) != vx(prev)) & live))
        nw += int(np.sum((w(f) != w(prev)) & live))
        resets += int(np.sum(st == 0))
        prev = f
    return nv, nw, resets


def run_case(name, kernel, monkeypatch):
    import torch
    from moog import environment
    from moog_demos import example_configs
    if kernel == 'generic':
        monkeypatch.setenv('MOOG_STEP_SPEC', '0')
    else:   # the specialised step kernels the build made (lib/spec)
        monkeypatch.delenv('MOOG_STEP_SPEC', raising=False)
        monkeypatch.delenv('MOOG_SPEC_DIR', raising=False)
    c = compiled(name)
    f0, q0, acts, F, Q, R, ST = oracle_run(name)
    seed = {'colliding_predators_32': 5, 'falling_balls_64': 5, 'colliding_predators': 11}[name]
    env = environment.BatchedEnvironment(num_envs=N, seed=seed, layer_capacity=example_configs.capacity(name),
                                         **example_configs.load(name))
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


@pytest.mark.parametrize('kernel', KERNELS)
def test_colliding_predators_32_free_running(kernel, monkeypatch):
    """The headline program over 40 calls in which every env times out and auto-resets once.  Oracle alone: 3664 sprite-calls
    with a changed x velocity, 4046 with a changed angular velocity, 16 auto-resets; the bar is one contact per env and call."""
    nv, nw, resets = contact_counts('colliding_predators_32')
    print('oracle: %d velocity changes, %d angular velocity changes, %d auto-resets' % (nv, nw, resets))
    assert nv >= 40 * N and nw >= 40 * N and resets == N
    run_case('colliding_predators_32', kernel, monkeypatch)


@pytest.mark.parametrize('kernel', KERNELS)
def test_falling_balls_64_pile_up_free_running(kernel, monkeypatch):
    """16 different recorded piles of 60 balls over 30 calls: dense candidate rows, several contacts per sub-step, mirrored
    pairs struck, re-tests that change rows ahead of the cursor.  Oracle alone: 1046 sprite-calls with a changed x velocity (a
    ball at rest in the pile keeps its x velocity of zero); the bar is one contact per env and call."""
    nv, nw, resets = contact_counts('falling_balls_64')
    print('oracle: %d velocity changes, %d auto-resets' % (nv, resets))
    assert nv >= 30 * N
    run_case('falling_balls_64', kernel, monkeypatch)


def test_spinning_predators_free_running(monkeypatch):
    """colliding_predators: float32 angular velocities, all non-zero at the start, that contacts change inside a sub-step
    (update_angle_vel=True), over 40 calls.  The build makes no specialised kernel for this program, so it runs on the generic
    kernel alone (the specialised binary meets spinning float32 sprites in colliding_predators_32 above).
    Oracle alone: 426 sprite-calls with a changed angular velocity; the bar is ten per env."""
    c = compiled('colliding_predators')
    P, L = c.program, c.layout
    f0, q0 = oracle_run('colliding_predators')[:2]
    s0, ns = P.layer_slot0[1], P.layer_nslots[1]
    assert np.all(q0[:, L.o_flags + s0:L.o_flags + s0 + ns] & helpers._abi.MOOG_F_ANGVEL_F32)
    assert np.all(f0[:, L.o_angvel + s0:L.o_angvel + s0 + ns] != 0)
    nv, nw, resets = contact_counts('colliding_predators')
    print('oracle: %d velocity changes, %d angular velocity changes' % (nv, nw))
    assert nw >= 10 * N
    run_case('colliding_predators', 'generic', monkeypatch)
