"""relative_motion_matrix (csrc/moog_device.h) evaluates the sines and cosines of a contact search's two rotation angles in one
pass of sincos_small -- lanes with bit 4 clear take the first angle, the others the second, and an exchange with lane ^ 16 hands
each lane the pair it did not compute -- instead of two passes in a row.  A lane's result depends on its own argument alone,
so results must not move by a bit.

CPU part (oracle only): the headline case holds what the change touches -- searches whose two sprites both turn by less than
2^-5 rad per sub-step (the Taylor branch in every lane), both by at least that (the library branch in every lane) and one of
each (both branches in one pass, the exchange across them).
GPU part: the one-pass form against the two calls in a row (debug word 2048) bit for bit on the generic kernel, and the
specialised and generic kernels free-running against the oracle at the bar of tests/test_step_contact_path.py (integers
exact, floats within 1e-5, no fault word).  One oracle trajectory per case and test session, shared by the tests and left
unchanged; the pile-up of falling_balls_64 is that file's case and trajectory, its first 20 calls."""
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

THRESHOLD = 2.0 ** -5   # sincos_small: Taylor series below, the library's sin and cos from here on
CLASS_FLOOR = 20        # searches of each class the headline case must hold

# colliding_predators_32: a seeded reset, PRED_LEAD oracle steps with random actions (the first contacts have spun the
# sprites up and most of them still spin fast), then the PRED_CALLS calls of the case.  Chosen on the CPU with the oracle
# alone; the counts are in test_searches_of_every_class_are_present's docstring.
PRED_SEED, PRED_LEAD, PRED_CALLS = 7, 20, 12
SEEDS = {'colliding_predators_32': PRED_SEED, 'falling_balls_64': 5}


def _frozen(out):
    f0, q0, acts, F, Q, R, ST = out
    for x in (f0, q0) + tuple(acts) + tuple(F) + tuple(Q) + tuple(R) + tuple(ST):
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def predators_oracle_run():
    """The oracle's trajectory of the headline case, shaped like contact_path.oracle_run's (read only)."""
    c = compiled('colliding_predators_32')
    o = helpers.OracleEnv(c, n_envs=N, seed=PRED_SEED)
    o.reset(render=False)
    rs = np.random.RandomState(3)
    for _ in range(PRED_LEAD):
        o.step(rs.uniform(-1, 1, size=(N, 2)), render=False)
    assert np.all(o.i32[:, c.layout.o_step_count] == PRED_LEAD)   # (no env has ended its episode on the way)
    f0, q0 = o.f64.copy(), o.i32.copy()
    acts, F, Q, R, ST = [], [], [], [], []
    for _ in range(PRED_CALLS):
        a = rs.uniform(-1, 1, size=(N, 2))
        o.step(a, render=False)
        acts.append(a); F.append(o.f64.copy()); Q.append(o.i32.copy()); R.append(o.reward.copy()); ST.append(o.step_type.copy())
    return _frozen((f0, q0, acts, F, Q, R, ST))


@functools.lru_cache(maxsize=None)
def falling_balls_oracle_run():
    """The recorded pile-up of tests/test_step_contact_path.py, the first 20 of its calls (that file's trajectory, read only)."""
    f0, q0, acts, F, Q, R, ST = contact_path.oracle_run('falling_balls_64')
    return (f0, q0, acts[:20], F[:20], Q[:20], R[:20], ST[:20])


def case(name):
    """(compiled program, its oracle trajectory)."""
    return compiled(name), (predators_oracle_run() if name == 'colliding_predators_32' else falling_balls_oracle_run())


CASES = ['colliding_predators_32', 'falling_balls_64']


# ---- CPU precondition -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def search_classes(name):
    """Every call of a case's trajectory again, from the oracle's own record before the call, one sub-step at a time with the
    oracle's search log on (as tests/test_step_batch_strikes.py::substep_survey reads it).  Every search the log records, at any
    depth of Collision.step's recursion, is classified by its two sprites' |angle_vel| / K in the record before the sub-step:
    returns the numbers of searches with (both below 2^-5, one of each, both at or above 2^-5)."""
    c, (f0, q0, acts, F, Q, R, ST) = case(name)
    L, K = c.layout, c.program.updates_per_env_step
    lib = helpers.oracle()
    o = helpers.OracleEnv(c, n_envs=N, seed=SEEDS[name])
    buf = np.zeros(1 << 20, np.int32)
    counts = np.zeros(3, np.int64)
    for t in range(len(acts)):
        o.f64[:], o.i32[:] = (f0, q0) if t == 0 else (F[t - 1], Q[t - 1])
        for _ in range(K):
            fast = np.abs(o.f64[:, L.o_angvel:L.o_angvel + L.S]) / K >= THRESHOLD   # (before the sub-step)
            lib.oracle_contact_log(buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(buf))
            o.physics(substep=True)
            m = lib.oracle_contact_log_count()
            lib.oracle_contact_log(None, 0)
            assert m < len(buf) - 2
            env = None
            for a, b in buf[:m].reshape(-1, 2):
                if a == -1:
                    env = int(b) - o.env_index0
                elif -5 <= a <= -3:   # the outcome of a search (CV_NONE, CV_OK, CV_FUTURE) of pair (b & 255, b >> 8 & 255)
                    counts[int(fast[env, int(b) & 255]) + int(fast[env, (int(b) >> 8) & 255])] += 1
    return tuple(int(x) for x in counts)


def test_searches_of_every_class_are_present():
    """colliding_predators_32 from step 20 of an episode over 12 calls (seed 7, 16 envs): at least 20 contact searches with
    both sprites below the threshold of sincos_small, 20 with both at or above it and 20 with one of each.  Oracle alone:
    899 below, 1094 of one each, 372 above."""
    below, mixed, above = search_classes('colliding_predators_32')
    print('colliding_predators_32: searches with both angles below 2^-5: %d, one of each: %d, both at or above: %d' % (below, mixed, above))
    assert below >= CLASS_FLOOR and mixed >= CLASS_FLOOR and above >= CLASS_FLOOR


def test_falling_balls_64_pile_up_holds_searches():
    """The pile-up has no class floor (its balls hardly spin); it must hold searches at all."""
    below, mixed, above = search_classes('falling_balls_64')
    print('falling_balls_64: searches with both angles below 2^-5: %d, one of each: %d, both at or above: %d' % (below, mixed, above))
    assert below + mixed + above >= CLASS_FLOOR


# ---- GPU --------------------------------------------------------------------------------------------------------------
def make_env(name):
    from moog import environment
    from moog_demos import example_configs
    return environment.BatchedEnvironment(num_envs=N, seed=SEEDS[name], layer_capacity=example_configs.capacity(name),
                                          **example_configs.load(name))


@gpu
@pytest.mark.parametrize('name', CASES)
def test_one_pass_equals_two_calls(name, monkeypatch):
    """The generic kernel with the one-pass form (debug word 0) and with the two calls of sincos_small in a row (2048) from the
    same records with the same actions: state records, rewards and step types bit-identical after every call, no fault word."""
    import torch
    monkeypatch.setenv('MOOG_STEP_SPEC', '0')
    c, (f0, q0, acts, F, Q, R, ST) = case(name)
    envs = []
    for dbg in (0, 2048):
        env = make_env(name)
        assert env.step_kernel() == 'generic', env.step_kernel()
        env.reset()
        env.state_f64.copy_(torch.from_numpy(np.array(f0)))
        env.state_i32.copy_(torch.from_numpy(np.array(q0)))
        env.check_faults = False
        env.set_debug(dbg, 0)
        envs.append(env)
    bits = lambda x: x.cpu().numpy().view(np.int64)
    for t, a in enumerate(acts):
        outs = [env.step(torch.from_numpy(np.array(a)).to(env.device)) for env in envs]
        torch.cuda.synchronize()
        assert np.array_equal(bits(envs[0].state_f64), bits(envs[1].state_f64)), 'float records differ at call %d' % t
        assert np.array_equal(envs[0].state_i32.cpu().numpy(), envs[1].state_i32.cpu().numpy()), 'integer records differ at call %d' % t
        assert np.array_equal(bits(outs[0].reward), bits(outs[1].reward)), 'rewards differ at call %d' % t
        assert np.array_equal(outs[0].step_type.cpu().numpy(), outs[1].step_type.cpu().numpy()), 'step types differ at call %d' % t
        assert not np.any(envs[0].state_i32.cpu().numpy()[:, c.layout.o_fault]), t
    for env in envs:
        env.close()


@gpu
@pytest.mark.parametrize('kernel', contact_path.KERNELS)
@pytest.mark.parametrize('name', CASES)
def test_against_the_oracle(name, kernel, monkeypatch):
    """contact_path.run_case for the cases of this file: free-running, never re-synchronised."""
    import torch
    c, (f0, q0, acts, F, Q, R, ST) = case(name)
    if kernel == 'generic':
        monkeypatch.setenv('MOOG_STEP_SPEC', '0')
    else:   # the specialised step kernels the build made (lib/spec)
        monkeypatch.delenv('MOOG_STEP_SPEC', raising=False)
        monkeypatch.delenv('MOOG_SPEC_DIR', raising=False)
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
