"""Action repeat (BatchedEnvironment(action_repeat=k), include/moog_engine.h moog_engine_set_action_repeat): k env-steps per
step() call inside one launch of the step kernel.

The judge is the CPU oracle, which has no repeat of its own: one oracle env per engine env is stepped with the call's
action once per repetition until its step type is LAST.  The engine's single-step path is the second witness: the state
after one repeat-k call must equal, bit for bit, the state after k single calls."""
import numpy as np
import pytest

import helpers
from moog import _abi

# (program, envs, seed, calls, step kernel asserted, natural episode ends asserted)
#   plain kernel with contacts | Grid actions | episodes that end by contact | Composite actions on the dynamic variant |
#   every component (+ Grid) | late reset | reset pool | a specialised workload
# `calls` and the seeds come from running expected_run() below on the oracle alone (no GPU) until the runs marked True hold
# envs whose episode ends strictly inside a repeat window (0 < m < k) AND envs that start a call with reset_next set by the
# task (the ones the test sets by hand, see FORCED, are not counted).  Observed (inside, starts) for k = 2 / 4 / 7:
#   chase_avoid_torus  (2, 8) / (12, 11) / (20, 16)
#   maze_zoo           (2, 2) / (6, 9) / (12, 15)
#   red_green_l1       (1, 2) / (1, 2) / (9, 9)
CASES = [('colliding_predators', 8, 3, 6, None, False),
         ('falling_balls', 8, 3, 6, None, False),
         ('chase_avoid_torus', 16, 3, 12, None, True),
         ('cleanup', 8, 3, 6, None, False),
         ('maze_zoo', 8, 5, 16, None, True),
         ('parallelogram_catch', 8, 3, 8, None, False),
         ('red_green_l1', 8, 5, 14, None, True),
         ('colliding_predators_32', 8, 3, 6, 'specialised', False)]
KS = (2, 4, 7)
FORCED = 2   # before this call, every fourth env (from env 1) gets reset_next set by hand: every program then has envs that
             # a repeat-k call must reset instead of stepping (parallelogram_catch: by the reset kernel behind the step kernel)


def draw_actions(P, n, rs):
    if P.n_actions > 1:   # Composite: [n, sub-spaces, 2]
        return rs.uniform(-1, 1, size=(n, P.n_actions, 2))
    if P.action.kind == _abi.MOOG_ACTION_GRID:
        return rs.randint(0, 5, size=n)
    return rs.uniform(-1, 1, size=(n, 2))


def oracle_call(o, L, a, k):
    """One call with action_repeat=k on a one-env oracle: (step_type, reward, discount, m) by the contract."""
    if o.i32[0, L.o_reset_next]:
        o.step(a, render=False)
        assert o.step_type[0] == 0
        return 0, np.nan, np.nan, 0
    total, m = None, 0
    for _ in range(k):
        o.step(a, render=False)
        r = float(o.reward[0])
        total = r if total is None else total + r   # ((r_1 + r_2) + ...) + r_m in float64
        m += 1
        if o.step_type[0] == 2:
            break
    return int(o.step_type[0]), total, float(o.discount[0]), m


def expected_run(name, n, seed, k, calls, env=None, check=None):
    """The run of test_repeat_vs_oracle on the oracle (alone when env is None: how CASES was chosen).  Returns the number of
    (env, call) pairs whose episode ended strictly inside the window and of those that started with reset_next set by the task."""
    c = env.compiled if env is not None else helpers.compiled(name)
    P, L = c.program, c.layout
    oracles = [helpers.OracleEnv(c, n_envs=1, seed=seed, env_index0=i) for i in range(n)]
    for o in oracles:
        o.reset(render=False)
    if env is not None:
        env.reset()
        check(-1, oracles, None, None)
    rs = np.random.RandomState(seed + 100 * k)
    inside = starts = 0
    for call in range(calls):
        a = draw_actions(P, n, rs)
        forced = np.zeros(n, bool)
        if call == FORCED:
            forced[1::4] = True
            for i in np.nonzero(forced)[0]:
                oracles[i].i32[0, L.o_reset_next] = 1
            if env is not None:
                env.state_i32[1::4, L.o_reset_next] = 1
        ts = env.step(a) if env is not None else None
        want = []
        for i, o in enumerate(oracles):
            natural = bool(o.i32[0, L.o_reset_next]) and not forced[i]
            want.append(oracle_call(o, L, a[i:i + 1], k))
            starts += int(natural)
            inside += int(0 < want[-1][3] < k)
        if env is not None:
            check(call, oracles, want, ts)
    return inside, starts


@pytest.mark.gpu
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('name,n,seed,calls,kernel,natural', CASES)
def test_repeat_vs_oracle(name, n, seed, calls, kernel, natural, k):
    """Per env against the oracle, after every call: step type, repeat count and the integer record exact; the float record
    <= 1e-9, reward and discount exact (the tolerances of test_gpu_parity.py::test_engine_vs_oracle_own_rng and smoke(),
    the two sides kept in lock step between calls as there); every frame bit-exact against the oracle's picture of the
    engine's own state."""
    import torch
    from test_gpu_parity import make_env, download
    env = make_env(name, n, seed=seed, action_repeat=k)
    if kernel is not None:
        assert env.step_kernel() == kernel
    painter = helpers.OracleEnv(env.compiled, n_envs=n, seed=seed)

    def check(call, oracles, want, ts):
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
            st, rw, dc, m = (np.array(x) for x in zip(*want))
            assert np.array_equal(ts.step_type.cpu().numpy(), st), call
            assert np.array_equal(env.repeat_count.cpu().numpy(), m), (call, env.repeat_count.cpu().numpy(), m)
            assert helpers.same_or_nan(ts.reward.cpu().numpy(), rw), (call, ts.reward.cpu().numpy(), rw)
            assert helpers.same_or_nan(ts.discount.cpu().numpy(), dc), call
            painter.f64[:], painter.i32[:] = f, q
            assert np.array_equal(ts.observation['image'].cpu().numpy(), painter.render()), 'call %d: frames differ' % call
        for i, o in enumerate(oracles):   # lock step (removes 1-ulp libm / ocml drift)
            o.f64[0], o.i32[0] = f[i], q[i]

    inside, starts = expected_run(name, n, seed, k, calls, env=env, check=check)
    torch.cuda.synchronize()
    env.close()
    if natural:
        assert inside > 0 and starts > 0, (inside, starts)


@pytest.mark.gpu
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('name,n,seed,macro', [('colliding_predators', 32, 7, 4), ('cleanup', 32, 7, 4),
                                               ('colliding_predators_32', 32, 7, 4), ('parallelogram_catch', 32, 7, 4)])
def test_repeat_equals_single_calls_bit_for_bit(name, n, seed, macro, k):
    """Two engines, same seed: B (action_repeat=1) makes k calls per macro-step, A (action_repeat=k) one.  On a window in
    which no episode ends (checked on the oracle first), after every macro-step both state tensors, the rewards summed in
    call order and the frames are equal bit for bit: any difference in box rebuilds, random-stream use or store order shows."""
    import torch
    from test_gpu_parity import make_env
    c = helpers.compiled(name)
    P = c.program
    rs = np.random.RandomState(seed)
    acts = [draw_actions(P, n, rs) for _ in range(macro)]
    o = helpers.OracleEnv(c, n_envs=n, seed=seed)
    o.reset(render=False)
    for a in acts:
        for _ in range(k):
            o.step(a, render=False)
            assert (o.step_type == 1).all(), 'an episode ends inside the window: pick another seed'
    A = make_env(name, n, seed=seed, action_repeat=k)
    B = make_env(name, n, seed=seed)
    assert A.action_repeat == k and B.action_repeat == 1
    A.reset()
    B.reset()
    assert torch.equal(A.state_f64, B.state_f64) and torch.equal(A.state_i32, B.state_i32)
    for i, a in enumerate(acts):
        ta = A.step(a)
        total = None
        for _ in range(k):
            tb = B.step(a)
            total = tb.reward.clone() if total is None else total + tb.reward
        assert torch.equal(A.state_i32, B.state_i32), i
        assert torch.equal(A.state_f64.view(torch.int64), B.state_f64.view(torch.int64)), i
        assert torch.equal(ta.reward.view(torch.int64), total.view(torch.int64)), i
        assert torch.equal(ta.step_type, tb.step_type) and torch.equal(ta.discount, tb.discount), i
        assert bool((A.repeat_count == k).all()) and bool((B.repeat_count == 1).all()), i
        assert torch.equal(ta.observation['image'], tb.observation['image']), i
    A.close()
    B.close()


@pytest.mark.gpu
def test_repeat_one_is_the_default_and_the_setter_takes_effect_at_the_next_call():
    import torch
    from test_gpu_parity import make_env
    n = 32
    env = make_env('chase_avoid_torus', n, seed=9)
    ref = make_env('chase_avoid_torus', n, seed=9, action_repeat=1)
    assert env.action_repeat == 1
    rs = np.random.RandomState(1)
    env.reset()
    ref.reset()
    assert bool((env.repeat_count == 0).all())
    firsts = 0
    for _ in range(40):   # (episodes of this program end by contact: FIRST timesteps occur)
        a = rs.uniform(-1, 1, size=(n, 2))
        t, r = env.step(a), ref.step(a)
        first = t.step_type == 0
        firsts += int(first.sum())
        assert torch.equal(env.repeat_count, torch.where(first, 0, 1).to(torch.int32))
        assert torch.equal(t.step_type, r.step_type) and torch.equal(env.state_i32, ref.state_i32)
        assert torch.equal(env.state_f64.view(torch.int64), ref.state_f64.view(torch.int64))
        assert torch.equal(t.observation['image'], r.observation['image'])
    assert firsts > 0
    # from here on env repeats 3 times per call, ref is called 3 times (envs whose episode ends inside a window aside)
    env.set_action_repeat(3)
    assert env.action_repeat == 3
    a = rs.uniform(-1, 1, size=(n, 2))
    running = ~env.reset_next_step.clone()
    t = env.step(a)
    for _ in range(3):
        ref.step(a)
    whole = running & (env.repeat_count == 3)
    assert int(whole.sum()) > 0
    assert bool((env.repeat_count[~running] == 0).all())
    assert torch.equal(env.state_i32[whole], ref.state_i32[whole])
    assert torch.equal(env.state_f64[whole].view(torch.int64), ref.state_f64[whole].view(torch.int64))
    env.set_action_repeat(1)
    env.step(a)
    assert bool((env.repeat_count <= 1).all())
    with pytest.raises(ValueError):
        env.set_action_repeat(0)
    with pytest.raises(ValueError):
        env.set_action_repeat(_abi.MOOG_MAX_ACTION_REPEAT + 1)
    with pytest.raises(NotImplementedError, match='injected_uniforms'):
        env.set_action_repeat(2)
        env.step(a, injected_uniforms=np.zeros((n, 4)))
    env.close()
    ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize('k', [2, 4])
def test_sub_batches_repeat_like_one_batch(k):
    """SubBatchedEnvironment(action_repeat=k) == BatchedEnvironment(action_repeat=k) on the same seeds, episode ends included."""
    import torch
    from moog import environment
    from moog_demos import example_configs
    n, G = 64, 4
    cfg = example_configs.load('chase_avoid_torus')
    one = environment.BatchedEnvironment(num_envs=n, seed=13, action_repeat=k, **cfg)
    sub = environment.SubBatchedEnvironment(num_envs=n, sub_batches=G, seed=13, action_repeat=k, **example_configs.load('chase_avoid_torus'))
    assert sub.action_repeat == k
    one.reset()
    sub.reset()
    rs = np.random.RandomState(2)
    short = 0
    for i in range(20):
        a = torch.as_tensor(rs.uniform(-1, 1, size=(n, 2)), device='cuda')
        t1, t2 = one.step(a), sub.step(a)
        torch.cuda.synchronize()
        assert torch.equal(one.repeat_count, sub.repeat_count), i
        short += int(((one.repeat_count > 0) & (one.repeat_count < k)).sum())
        assert torch.equal(one.state_i32, sub.state_i32) and torch.equal(one.state_f64.view(torch.int64), sub.state_f64.view(torch.int64)), i
        assert torch.equal(t1.step_type, t2.step_type), i
        assert torch.equal(t1.reward.view(torch.int64), t2.reward.view(torch.int64)), i
        assert torch.equal(t1.observation['image'], t2.observation['image']), i
    assert short > 0, 'no episode ended inside a window'
    one.close()
    sub.close()


def _meta_config():
    """A config with a host-side rule and a meta_state_initializer (needs no device to build)."""
    from moog import game_rules
    from moog_demos import example_configs
    cfg = example_configs.load('pong')
    cfg['game_rules'] = tuple(cfg.get('game_rules', ())) + (game_rules.ModifyMetaState(lambda meta: meta.update(n=meta['n'] + 1)),)
    cfg['meta_state_initializer'] = lambda: {'n': 0}
    return cfg


def test_refusals_need_no_device():
    """What cannot be repeated on the device is refused at construction, with the reason, before anything touches a device:
    host-side meta-state rules, a meta_state_initializer, layer_capacity='auto'; and k outside 1 .. MOOG_MAX_ACTION_REPEAT."""
    from moog import environment
    from moog_demos import example_configs
    with pytest.raises(NotImplementedError, match='host-side meta-state rules'):
        environment.BatchedEnvironment(num_envs=4, action_repeat=2, **_meta_config())
    cfg = example_configs.load('pong')
    cfg['meta_state_initializer'] = lambda: {'n': 0}
    with pytest.raises(NotImplementedError, match='meta_state_initializer'):
        environment.BatchedEnvironment(num_envs=4, action_repeat=3, **cfg)
    for cap in ('auto', {'auto': True, 'prey': 16}):
        with pytest.raises(NotImplementedError, match="layer_capacity='auto'"):
            environment.BatchedEnvironment(num_envs=4, action_repeat=2, layer_capacity=cap, **example_configs.load('rules_zoo'))
    for bad in (0, -1, _abi.MOOG_MAX_ACTION_REPEAT + 1, 2.5, True):
        with pytest.raises(ValueError, match='action_repeat must be an integer'):
            environment.BatchedEnvironment(num_envs=4, action_repeat=bad, **example_configs.load('pong'))
    with pytest.raises(NotImplementedError, match='host-side meta-state rules'):
        environment.Environment(action_repeat=2, **_meta_config())


def test_abi_declares_the_setter_and_leaves_the_programs_alone():
    """ABI 31 = ABI 30 + moog_engine_set_action_repeat; the program blob keeps its own version number, so program bytes --
    hence hashes and the names of the specialised step kernels -- do not move with the entry point."""
    import ctypes
    from moog import _engine
    assert _abi.MOOG_ABI_VERSION == 31 and _abi.MOOG_PROGRAM_VERSION == 30 and _abi.MOOG_MAX_ACTION_REPEAT >= 8
    assert 'moog_engine_set_action_repeat' in _engine.SYMBOLS
    lib = _engine.load_library()
    assert lib.moog_engine_set_action_repeat(None, 2, None) != 0   # (a null engine is refused, not dereferenced)
    P = helpers.compiled('colliding_predators_32').program
    assert P.abi_version == _abi.MOOG_PROGRAM_VERSION
    h = ctypes.c_uint64()
    _engine.check(lib, lib.moog_program_step_kernel(ctypes.byref(P), None, None, ctypes.byref(h)))
    assert '%016x' % h.value == '417c47560f31861d'   # (the headline's specialised kernel: tests/test_host.py names its object)
