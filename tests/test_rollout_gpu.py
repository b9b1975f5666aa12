"""Open-loop rollouts (BatchedEnvironment.rollout, include/moog_engine.h moog_engine_step_sequence): T env-steps with T
different actions inside one launch of the step kernel, the reward of every step returned.

Two witnesses, as for the action repeat (test_action_repeat.py): the engine's own single-step path -- the state after
rollout(acts[0:T]) must equal, bit for bit, the state after step(acts[0]) ... step(acts[T - 1]) -- and the CPU oracle, one
one-env oracle per engine env stepped with the call's per-step actions until its step type is LAST."""
import numpy as np
import pytest

import helpers
from moog import _abi
from test_action_repeat import draw_actions

pytestmark = pytest.mark.gpu

FORCED = 2   # before this call every fourth env (from env 1) gets reset_next set by hand (test_action_repeat.FORCED)


def draw_sequence(P, n, T, rs):
    """[T, n, ...]: one draw_actions block per env-step."""
    return np.stack([draw_actions(P, n, rs) for _ in range(T)])


# -- 1. bit for bit against single calls ------------------------------------------------------------------------------
# (program, seed, step kernel asserted, float32 actions): 32 envs, 4 macro-steps; the seeds come from running window_is_quiet()
# on the oracle alone until no episode ends in the 32 env-steps of T = 8 (the shorter windows are prefixes of it: the per-step
# actions are one stream, cut into calls of T)
EQUAL_CASES = [('colliding_predators', 7, None, False),
               ('colliding_predators', 7, None, True),
               ('cleanup', 7, None, False),
               ('maze_zoo', 104, None, False),
               ('parallelogram_catch', 7, None, False),
               ('colliding_predators_32', 7, 'specialised', False)]
EQUAL_N, EQUAL_MACRO = 32, 4
# maze_zoo: with uniform moves a ghost catches the agent of one of 32 envs within 32 env-steps on every seed in 1 .. 6000 (31
# quiet steps at best); the agent that never moves up (move 3) has quiet windows, seed 104 the first
MAZE_MOVES = np.array([0, 1, 2, 4])


def equal_actions(name, seed, T, f32):
    P = helpers.compiled(name).program
    rs = np.random.RandomState(seed)
    if name == 'maze_zoo':
        return MAZE_MOVES[rs.randint(0, len(MAZE_MOVES), size=(T * EQUAL_MACRO, EQUAL_N))]
    acts = draw_sequence(P, EQUAL_N, T * EQUAL_MACRO, rs)
    return acts.astype(np.float32) if f32 else acts


def window_is_quiet(name, seed, T, f32=False):
    """The oracle alone: no episode ends in the window the bit-for-bit test runs."""
    c = helpers.compiled(name)
    o = helpers.OracleEnv(c, n_envs=EQUAL_N, seed=seed)
    o.reset(render=False)
    for a in equal_actions(name, seed, T, f32):
        o.step(a, render=False)
        if not (o.step_type == 1).all():
            return False
    return True


@pytest.mark.parametrize('T', [1, 3, 8])
@pytest.mark.parametrize('name,seed,kernel,f32', EQUAL_CASES)
def test_rollout_equals_single_calls_bit_for_bit(name, seed, kernel, f32, T):
    """Two engines, same seed: A makes one rollout of T actions per macro-step, B T single step() calls.  After every
    macro-step both state tensors, every per-step reward, their in-order sum, step type, discount, count and the frame are
    equal (the floats as bits)."""
    import torch
    from test_gpu_parity import make_env
    assert window_is_quiet(name, seed, T, f32), 'an episode ends inside the window: pick another seed'
    acts = equal_actions(name, seed, T, f32)
    A = make_env(name, EQUAL_N, seed=seed)
    B = make_env(name, EQUAL_N, seed=seed)
    if kernel is not None:
        assert A.step_kernel() == kernel and B.step_kernel() == kernel
    A.reset()
    B.reset()
    assert torch.equal(A.state_f64, B.state_f64) and torch.equal(A.state_i32, B.state_i32)
    bits = lambda t: t.view(torch.int64)   # noqa: E731
    for i in range(EQUAL_MACRO):
        seq = acts[i * T:(i + 1) * T]
        ta, rewards, count = A.rollout(seq)
        assert rewards.shape == (T, EQUAL_N) and rewards.dtype == torch.float64
        total = None
        for t in range(T):
            tb = B.step(seq[t])
            assert torch.equal(bits(rewards[t]), bits(tb.reward)), (i, t)
            total = tb.reward.clone() if total is None else total + tb.reward
        assert torch.equal(A.state_i32, B.state_i32), i
        assert torch.equal(bits(A.state_f64), bits(B.state_f64)), i
        assert torch.equal(bits(ta.reward), bits(total)), i
        assert torch.equal(ta.step_type, tb.step_type) and torch.equal(bits(ta.discount), bits(tb.discount)), i
        assert count is A.repeat_count and bool((count == T).all()), i
        assert torch.equal(ta.observation['image'], tb.observation['image']), i
    A.close()
    B.close()


# -- 2. against the oracle, episode ends included ------------------------------------------------------------------------
# (program, envs, seed, calls, natural episode ends asserted)
# `calls` and the seeds come from running expected_run() on the oracle alone (no GPU) until the runs marked True hold envs
# whose episode ends strictly inside a window (0 < m < T) AND envs that start a call with reset_next set by the task (the
# ones the test sets by hand are not counted).  Observed (inside, starts) for T = 2 / 5 / 8:
#   chase_avoid_torus  (3, 5) / (15, 16) / (23, 19)
#   maze_zoo           (2, 1) / (5, 10) / (12, 13)
#   red_green_l1       (1, 1) / (2, 3) / (6, 7)
# (the seeds of test_action_repeat.CASES do not carry over -- the actions differ per step: maze_zoo at its seed 5 has no
#  episode end inside a window of 2)
ORACLE_CASES = [('chase_avoid_torus', 16, 3, 12, True),
                ('maze_zoo', 8, 1, 16, True),
                ('red_green_l1', 8, 5, 14, True),
                ('parallelogram_catch', 8, 3, 8, False)]
TS = (2, 5, 8)


def oracle_rollout(o, L, seq):
    """One rollout of the actions seq [T, 1, ...] on a one-env oracle: (step_type, reward, discount, m, per-step rewards
    [T], zero behind m) by the contract."""
    per_step = np.zeros(len(seq))
    if o.i32[0, L.o_reset_next]:
        o.step(seq[0], render=False)
        assert o.step_type[0] == 0
        return 0, np.nan, np.nan, 0, per_step
    total, m = None, 0
    for a in seq:
        o.step(a, render=False)
        r = float(o.reward[0])
        per_step[m] = r
        total = r if total is None else total + r   # ((r_1 + r_2) + ...) + r_m in float64
        m += 1
        if o.step_type[0] == 2:
            break
    return int(o.step_type[0]), total, float(o.discount[0]), m, per_step


def expected_run(name, n, seed, T, calls, env=None, check=None):
    """The run of test_rollout_vs_oracle on the oracle (alone when env is None: how ORACLE_CASES was chosen).  Returns the
    number of (env, call) pairs whose episode ended strictly inside the window and of those that started with reset_next set
    by the task."""
    c = env.compiled if env is not None else helpers.compiled(name)
    P, L = c.program, c.layout
    oracles = [helpers.OracleEnv(c, n_envs=1, seed=seed, env_index0=i) for i in range(n)]
    for o in oracles:
        o.reset(render=False)
    if env is not None:
        env.reset()
        check(-1, oracles, None, None)
    rs = np.random.RandomState(seed + 100 * T)
    inside = starts = 0
    for call in range(calls):
        seq = draw_sequence(P, n, T, rs)
        forced = np.zeros(n, bool)
        if call == FORCED:
            forced[1::4] = True
            for i in np.nonzero(forced)[0]:
                oracles[i].i32[0, L.o_reset_next] = 1
            if env is not None:
                env.state_i32[1::4, L.o_reset_next] = 1
        got = env.rollout(seq) if env is not None else None
        want = []
        for i, o in enumerate(oracles):
            natural = bool(o.i32[0, L.o_reset_next]) and not forced[i]
            want.append(oracle_rollout(o, L, seq[:, i:i + 1]))
            starts += int(natural)
            inside += int(0 < want[-1][3] < T)
            if forced[i]:
                assert want[-1][3] == 0 and not want[-1][4].any()
        if env is not None:
            check(call, oracles, want, got)
    return inside, starts


@pytest.mark.parametrize('T', TS)
@pytest.mark.parametrize('name,n,seed,calls,natural', ORACLE_CASES)
def test_rollout_vs_oracle(name, n, seed, calls, natural, T):
    """Per env against the oracle, after every call: step type, count and the integer record exact; the float record <= 1e-9;
    the timestep's reward and discount exact; rewards[:m] exactly the oracle's per-step rewards and rewards[m:] exactly 0.0
    (the whole column of an env the call reset); every frame bit-exact against the oracle's picture of the engine's own
    state.  The two sides are put in lock step between calls (test_action_repeat.py::test_repeat_vs_oracle)."""
    import torch
    from test_gpu_parity import make_env, download
    env = make_env(name, n, seed=seed)
    painter = helpers.OracleEnv(env.compiled, n_envs=n, seed=seed)

    def check(call, oracles, want, got):
        f, q = download(env)
        of = np.concatenate([o.f64 for o in oracles])
        oq = np.concatenate([o.i32 for o in oracles])
        assert np.array_equal(q, oq), 'call %d: integer records differ in envs %s' % (call, np.nonzero((q != oq).any(1))[0][:8])
        with np.errstate(invalid='ignore'):
            err = np.abs(f - of)
        err = np.where(np.isnan(f) & np.isnan(of), 0, err)
        err = np.where(f == of, 0, err)
        assert float(np.max(err)) <= 1e-9, (call, float(np.max(err)))
        if want is not None:
            ts, rewards, count = got
            st, rw, dc, m, per_step = (np.array(x) for x in zip(*want))
            assert np.array_equal(ts.step_type.cpu().numpy(), st), call
            assert np.array_equal(count.cpu().numpy(), m), (call, count.cpu().numpy(), m)
            assert helpers.same_or_nan(ts.reward.cpu().numpy(), rw), (call, ts.reward.cpu().numpy(), rw)
            assert helpers.same_or_nan(ts.discount.cpu().numpy(), dc), call
            r = rewards.cpu().numpy()
            assert r.shape == (T, n)
            assert np.array_equal(r.view(np.int64), per_step.T.copy().view(np.int64)), (call, r, per_step.T)
            for i in range(n):
                assert not r[m[i]:, i].any() and not np.signbit(r[m[i]:, i]).any(), (call, i)
            if call == FORCED:
                assert (m[1::4] == 0).all() and not r[:, 1::4].any()
            painter.f64[:], painter.i32[:] = f, q
            assert np.array_equal(ts.observation['image'].cpu().numpy(), painter.render()), 'call %d: frames differ' % call
        for i, o in enumerate(oracles):   # lock step (removes 1-ulp libm / ocml drift)
            o.f64[0], o.i32[0] = f[i], q[i]

    inside, starts = expected_run(name, n, seed, T, calls, env=env, check=check)
    torch.cuda.synchronize()
    env.close()
    if natural:
        assert inside > 0 and starts > 0, (inside, starts)


# -- 3. the engine is left as it was found ----------------------------------------------------------------------------------
def test_rollout_leaves_the_engine_as_it_found_it():
    """step() before and after a rollout, and set_action_repeat(3) after it, behave as on an engine that never rolled out:
    state bits against a twin that reaches the same states by single calls."""
    import torch
    from test_gpu_parity import make_env
    n, T = 32, 4
    name, seed = 'colliding_predators', 7
    assert window_is_quiet(name, seed, 8)   # (the same action stream: 2 + 4 + 2 + 3 env-steps of its 32)
    acts = equal_actions(name, seed, 8, False)
    env, twin = make_env(name, n, seed=seed), make_env(name, n, seed=seed)
    env.reset()
    twin.reset()

    def same(where):
        assert torch.equal(env.state_i32, twin.state_i32), where
        assert torch.equal(env.state_f64.view(torch.int64), twin.state_f64.view(torch.int64)), where

    for t in range(2):
        ta, tb = env.step(acts[t]), twin.step(acts[t])
    same('before')
    assert env.action_repeat == 1
    _, rewards, count = env.rollout(acts[2:2 + T])
    for t in range(2, 2 + T):
        twin.step(acts[t])
    same('rollout')
    assert env.action_repeat == 1 and bool((count == T).all())
    for t in range(6, 8):   # a step() after the call takes ONE env-step
        ta, tb = env.step(acts[t]), twin.step(acts[t])
        assert bool((env.repeat_count == 1).all())
        assert torch.equal(ta.reward.view(torch.int64), tb.reward.view(torch.int64))
        assert torch.equal(ta.observation['image'], tb.observation['image'])
    same('after')
    env.set_action_repeat(3)
    env.step(acts[8])
    for _ in range(3):
        twin.step(acts[8])
    assert bool((env.repeat_count == 3).all())
    same('repeat')
    env.close()
    twin.close()


# -- 4. sub-batches -----------------------------------------------------------------------------------------------------------
def test_sub_batches_roll_out_like_one_batch():
    """SubBatchedEnvironment.rollout == BatchedEnvironment.rollout on the same seeds, episode ends included."""
    import torch
    from moog import environment
    from moog_demos import example_configs
    n, G, T = 64, 4, 4
    one = environment.BatchedEnvironment(num_envs=n, seed=13, **example_configs.load('chase_avoid_torus'))
    sub = environment.SubBatchedEnvironment(num_envs=n, sub_batches=G, seed=13, **example_configs.load('chase_avoid_torus'))
    one.reset()
    sub.reset()
    rs = np.random.RandomState(2)
    short = 0
    for i in range(20):
        a = torch.as_tensor(rs.uniform(-1, 1, size=(T, n, 2)), device='cuda')
        (t1, r1, c1), (t2, r2, c2) = one.rollout(a), sub.rollout(a)
        torch.cuda.synchronize()
        assert r2.shape == (T, n) and torch.equal(c1, c2), i
        short += int(((c1 > 0) & (c1 < T)).sum())
        assert torch.equal(one.state_i32, sub.state_i32) and torch.equal(one.state_f64.view(torch.int64), sub.state_f64.view(torch.int64)), i
        assert torch.equal(r1.view(torch.int64), r2.view(torch.int64)), i
        assert torch.equal(t1.step_type, t2.step_type), i
        assert torch.equal(t1.observation['image'], t2.observation['image']), i
    assert short > 0, 'no episode ended inside a window'
    one.close()
    sub.close()


# -- 5. refusals that need an env ----------------------------------------------------------------------------------------
def test_refusals_leave_the_env_stepping():
    import torch
    from test_gpu_parity import make_env
    n = 8
    rs = np.random.RandomState(0)
    env = make_env('colliding_predators', n, seed=1)
    env.reset()
    for bad_T in (0, _abi.MOOG_MAX_ACTION_REPEAT + 1):
        with pytest.raises(ValueError, match='1 .. %d' % _abi.MOOG_MAX_ACTION_REPEAT):
            env.rollout(np.zeros((bad_T, n, 2)))
        env.step(rs.uniform(-1, 1, size=(n, 2)))
    with pytest.raises(ValueError, match=r'\[T, 8, 2\]'):
        env.rollout(np.zeros((2, n, 3)))
    env.step(rs.uniform(-1, 1, size=(n, 2)))
    env.set_action_repeat(2)
    with pytest.raises(NotImplementedError, match='action_repeat=2'):
        env.rollout(np.zeros((2, n, 2)))
    env.step(rs.uniform(-1, 1, size=(n, 2)))
    assert bool((env.repeat_count == 2).all())
    env.set_action_repeat(1)
    _, rewards, count = env.rollout(rs.uniform(-1, 1, size=(2, n, 2)))
    assert bool((count == 2).all()) and rewards.shape == (2, n)
    env.close()

    grid = make_env('maze_zoo', n, seed=1)
    grid.reset()
    with pytest.raises(ValueError, match=r'\[T, 8\]'):
        grid.rollout(np.zeros((2, n, 2)))
    grid.step(rs.randint(0, 5, size=n))
    grid.close()

    comp = make_env('cleanup', n, seed=1)
    comp.reset()
    keys = list(comp.action_space.action_keys)
    assert len(keys) > 1
    with pytest.raises(ValueError, match='composite action keys'):
        comp.rollout({k: np.zeros((2, n, 2)) for k in keys[:-1]})
    with pytest.raises(ValueError, match=r'\[T, 8, %d, 2\]' % len(keys)):
        comp.rollout(np.zeros((2, n, len(keys) + 1, 2)))
    comp.step(rs.uniform(-1, 1, size=(n, len(keys), 2)))
    # (the dict form and the packed form are one sequence)
    twin = make_env('cleanup', n, seed=1)
    twin.reset()
    twin.step(comp._last_action.reshape(n, len(keys), 2))
    seq = rs.uniform(-1, 1, size=(3, n, len(keys), 2))
    _, r1, _ = comp.rollout({k: seq[:, :, i] for i, k in enumerate(keys)})
    _, r2, _ = twin.rollout(seq)
    assert torch.equal(comp.state_f64.view(torch.int64), twin.state_f64.view(torch.int64)) and torch.equal(r1, r2)
    comp.close()
    twin.close()
