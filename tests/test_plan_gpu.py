"""Candidate rollouts on the MI355X (BatchedEnvironment.rollout_candidates, include/moog_engine.h moog_engine_plan_sequences):
K action sequences of T env-steps per env from the live state, one launch, nothing written back.

The witness is the engine's own rollout() on a twin engine B of the same seed, built without a reset pool: clone both state
tensors, rollout(actions[k]), copy both tensors back raw (random counters included), for each k.  Every comparison is on
bits; there is no tolerance anywhere."""
import numpy as np
import pytest

import helpers
import test_rollout_gpu as ro
from moog import _abi
from test_action_repeat import draw_actions

pytestmark = pytest.mark.gpu


def b64(t):
    import torch
    return t.view(torch.int64)


def draw_candidates(P, n, K, T, rs, name=None):
    """[K, T, n, ...]: one draw_actions block per candidate and env-step (maze_zoo: the moves of ro.MAZE_MOVES)."""
    if name == 'maze_zoo':
        return ro.MAZE_MOVES[rs.randint(0, len(ro.MAZE_MOVES), size=(K, T, n))]
    return np.stack([np.stack([draw_actions(P, n, rs) for _ in range(T)]) for _ in range(K)])


def snapshot(env):
    import torch
    torch.cuda.synchronize()
    return env.state_f64.clone(), env.state_i32.clone()


def put_back(env, snap):
    env.state_f64.copy_(snap[0])
    env.state_i32.copy_(snap[1])


def witness(B, acts, record=None):
    """What rollout_candidates(acts) must return, from K rollouts of the twin B, each from B's present state:
    (rewards [K, T, n], count [K, n], ended [K, n], {key: [K, T, n, rows, columns]}, the records after each rollout)."""
    import torch
    snap = snapshot(B)
    rewards, count, ended, traj, after = [], [], [], [], []
    for k in range(len(acts)):
        out = B.rollout(acts[k], record=record)
        torch.cuda.synchronize()
        rewards.append(out[1].clone())
        count.append(out[2].clone())
        ended.append((out[0].step_type == 2).to(torch.uint8))
        if record is not None:
            traj.append({key: t.clone() for key, t in out[3].items()})
        after.append(snapshot(B))
        put_back(B, snap)
    tr = {key: torch.stack([t[key] for t in traj]) for key in traj[0]} if traj else None
    return torch.stack(rewards), torch.stack(count), torch.stack(ended), tr, after


def assert_same(got, want, where):
    import torch
    rewards, count, ended = got[:3]
    assert rewards.dtype == torch.float64 and count.dtype == torch.int32 and ended.dtype == torch.uint8, where
    assert rewards.shape == want[0].shape and count.shape == want[1].shape and ended.shape == want[2].shape, where
    assert torch.equal(count, want[1]), (where, count, want[1])
    assert torch.equal(ended, want[2]), (where, ended, want[2])
    assert torch.equal(b64(rewards), b64(want[0])), (where, int((b64(rewards) != b64(want[0])).sum()))


def twins(name, n, seed, warm=3, f32=False, **kw):
    """A (plans) and B (the witness, no reset pool) after a reset and `warm` common steps."""
    import torch
    from test_gpu_parity import make_env
    A = make_env(name, n, seed=seed, **kw)
    B = make_env(name, n, seed=seed, reset_pool=False, **kw)
    A.reset()
    B.reset()
    rs = np.random.RandomState(seed + 17)
    P = A.compiled.program
    for _ in range(warm):
        a = draw_candidates(P, n, 1, 1, rs, name)[0, 0]
        a = a.astype(np.float32) if f32 else a
        A.step(a)
        B.step(a)
    assert torch.equal(A.state_i32, B.state_i32) and torch.equal(b64(A.state_f64), b64(B.state_f64))
    return A, B, rs


# -- 1. equal to K rollouts -------------------------------------------------------------------------------------------------
# (program, seed, plan kernel asserted, float32 actions, K, N, Ts)
EQUAL_CASES = [('colliding_predators', 7, None, False, 3, 5, (1, 5, 8)),
               ('colliding_predators', 7, None, True, 3, 5, (5,)),
               ('colliding_predators', 7, None, False, 1, 5, (5,)),
               ('cleanup', 7, None, False, 3, 5, (1, 5, 8)),
               ('rules_zoo', 7, None, False, 3, 5, (1, 5, 8)),   # (the cut fields: see CUT_PROGRAM)
               ('maze_zoo', 104, None, False, 3, 5, (1, 5, 8)),
               ('parallelogram_catch', 7, None, False, 3, 5, (1, 5, 8)),
               ('colliding_predators_32', 7, 'specialised', False, 3, 5, (1, 5, 8)),
               ('pong', 3, None, False, 2, 4, (64,))]   # (T = 64: the lane-per-step zeroing of the steps not taken)


# The program that exercises the fields hot_layout() cuts out of the staged record.  cleanup does not: its 31 slots are an odd
# number, so its colours are never cut, and on the oracle no colour or opacity word of it changes before step 36 of this
# stream.  rules_zoo (18 slots, colours cut) changes colour / opacity words in the first window; the test asserts it.
CUT_PROGRAM = 'rules_zoo'


@pytest.mark.parametrize('name,seed,kernel,f32,K,n,Ts', EQUAL_CASES)
def test_candidates_equal_k_rollouts_bit_for_bit(name, seed, kernel, f32, K, n, Ts):
    import torch
    A, B, rs = twins(name, n, seed, f32=f32)
    L, S = A.layout, A.layout.S
    if kernel is not None:
        assert A.plan_kernel() == kernel, A.plan_kernel()
    print(name, 'plans with the', A.plan_kernel(), 'kernel')
    cut_moved = False
    for T in Ts:
        acts = draw_candidates(A.compiled.program, n, K, T, rs, name)
        acts = acts.astype(np.float32) if f32 else acts
        before = snapshot(B)
        want = witness(B, acts)
        for f, q in want[4]:   # (the fields the step kernels keep out of LDS: colours; opacities, shape ids, Portal bits)
            cut_moved = cut_moved or not torch.equal(b64(f[:, L.o_color:L.o_color + 3 * S]), b64(before[0][:, L.o_color:L.o_color + 3 * S]))
            cut_moved = cut_moved or not torch.equal(q[:, L.o_opacity:L.o_opacity + S], before[1][:, L.o_opacity:L.o_opacity + S])
        got = A.rollout_candidates(acts)
        torch.cuda.synchronize()
        assert len(got) == 3 and got[0].shape == (K, T, n)
        assert_same(got, want, (name, T))
        assert torch.equal(A.state_i32, B.state_i32) and torch.equal(b64(A.state_f64), b64(B.state_f64)), T
    if name == CUT_PROGRAM:
        assert S % 2 == 0 and cut_moved, 'the witness rollouts change no colour or opacity word: pick a program that does'
    A.close()
    B.close()


# -- 2. episode ends --------------------------------------------------------------------------------------------------------
# (program, envs, seed, rounds): a round = one plan of K = 3 candidates of T = 5 steps, then one real step with candidate 0's
# first action.  The seeds and round counts come from running expected_ends() on the oracle alone (no GPU) until all three
# properties hold with room to spare; observed (inside, natural starts, envs whose candidates differ):
#   chase_avoid_torus  16 envs, seed 3, 24 rounds: (66, 5, 44)
#   red_green_l1        8 envs, seed 5, 120 rounds: (60, 5, 102)   (80 rounds: (24, 2, 59); its episodes are long)
ENDS_K, ENDS_T = 3, 5
ENDS_CASES = [('chase_avoid_torus', 16, 3, 24), ('red_green_l1', 8, 5, 120)]
FORCED_ROUND = 2   # before this round's plan every fourth env (from env 1) gets reset_next set by hand


def ends_actions(name, n, seed, rounds):
    P = helpers.compiled(name).program
    rs = np.random.RandomState(seed + 1000)
    return [draw_candidates(P, n, ENDS_K, ENDS_T, rs, name) for _ in range(rounds)]


def expected_ends(name, n, seed, rounds):
    """The run of test_episode_ends on one-env oracles alone: how ENDS_CASES was chosen.  Returns the number of (round, k, env)
    with 0 < count < T, of (round, env) that start a plan with reset_next set by the task, and of (round, env) whose
    candidates differ in count or in a reward's bits."""
    c = helpers.compiled(name)
    L = c.layout
    oracles = [helpers.OracleEnv(c, n_envs=1, seed=seed, env_index0=i) for i in range(n)]
    for o in oracles:
        o.reset(render=False)
    inside = starts = differ = 0
    for r, acts in enumerate(ends_actions(name, n, seed, rounds)):
        for i, o in enumerate(oracles):
            forced = r == FORCED_ROUND and i % 4 == 1
            if forced:
                o.i32[0, L.o_reset_next] = 1
            if o.i32[0, L.o_reset_next]:
                starts += int(not forced)
            else:
                f, q = o.f64.copy(), o.i32.copy()
                outs = []
                for k in range(ENDS_K):
                    st, _, _, m, per_step = ro.oracle_rollout(o, L, acts[k][:, i:i + 1])
                    outs.append((m, per_step.tobytes()))
                    inside += int(0 < m < ENDS_T)
                    o.f64[:], o.i32[:] = f, q
                differ += int(len(set(outs)) > 1)
            o.step(acts[0][0][i:i + 1], render=False)
    return inside, starts, differ


@pytest.mark.parametrize('name,n,seed,rounds', ENDS_CASES)
def test_episode_ends(name, n, seed, rounds):
    """Plans across episode ends: a candidate stops at the step that ends the episode (0 < count < T, ended = 1, zeros
    behind), an env whose reset_next is set takes no step in any candidate and is not reset, candidates of one env part ways.
    All three are asserted on the witness, and the plan equals it in every round."""
    import torch
    A, B, _ = twins(name, n, seed, warm=0)
    o = A.layout.o_reset_next
    inside = natural = differ = 0
    for r, acts in enumerate(ends_actions(name, n, seed, rounds)):
        forced = torch.zeros(n, dtype=torch.bool, device=A.state_i32.device)
        if r == FORCED_ROUND:
            forced[1::4] = True
            A.state_i32[1::4, o] = 1
            B.state_i32[1::4, o] = 1
        flagged = A.state_i32[:, o].clone() == 1
        want = witness(B, acts)
        before = snapshot(A)
        got = A.rollout_candidates(acts)
        assert_same(got, want, (name, r))
        assert torch.equal(A.state_i32, before[1]) and torch.equal(b64(A.state_f64), b64(before[0])), r
        rewards, count, ended = want[:3]
        assert bool((count[:, flagged] == 0).all()) and bool((count[:, ~flagged] > 0).all()), r
        assert not bool(rewards[:, :, flagged].any()) and not bool(ended[:, flagged].any()), r
        for k in range(ENDS_K):   # (behind the last step taken: exactly +0.0)
            steps = torch.arange(ENDS_T, device=count.device)[:, None]
            assert not bool(b64(rewards[k])[steps >= count[k][None, :].to(torch.int64)].any()), (r, k)
        assert bool((ended[(count > 0) & (count < ENDS_T)] == 1).all()) and bool((count[ended == 1] > 0).all()), r
        inside += int(((count > 0) & (count < ENDS_T)).sum())
        natural += int((flagged & ~forced).sum())
        differ += int(((count != count[0:1]).any(0) | (b64(rewards) != b64(rewards[0:1])).any(1).any(0)).sum())
        a0 = acts[0][0]
        A.step(a0)
        B.step(a0)
        assert torch.equal(A.state_i32, B.state_i32) and torch.equal(b64(A.state_f64), b64(B.state_f64)), r
    print(name, 'inside', inside, 'natural starts', natural, 'envs whose candidates differ', differ)
    assert inside > 0 and natural > 0 and differ > 0, (inside, natural, differ)
    A.close()
    B.close()


# -- 3. nothing changed ---------------------------------------------------------------------------------------------------------
# (program, envs, seed, real steps, steps before which every other env's episode is ended by hand on both twins).  From the
# oracle alone, with this test's action stream: colliding_predators' episodes end at its timeout (FIRST at steps 200 and 401),
# red_green_l1 (the pool program) opens episodes at steps 36, 50, 127, 155; parallelogram_catch (the late-reset program,
# timeout 500) ends none in 400 steps of random play, so its episodes are ended by hand, twice.
NOTHING_CASES = [('colliding_predators', 8, 7, 410, ()), ('parallelogram_catch', 6, 3, 60, (10, 35)), ('red_green_l1', 6, 5, 160, ())]


@pytest.mark.parametrize('name,n,seed,steps,forced', NOTHING_CASES)
def test_a_plan_leaves_nothing_behind(name, n, seed, steps, forced):
    """Both state tensors, the cost array, repeat_count and the last timestep's tensors are bit-equal before and after a call;
    then A, which plans before every step, and C, a twin that never does (default reset pool), take the same real steps, two
    episode lengths of them (NOTHING_CASES): state, reward, step type and frame stay equal throughout, across auto-resets,
    late resets and the pool's take-overs."""
    import torch
    from test_gpu_parity import make_env
    A, C = make_env(name, n, seed=seed), make_env(name, n, seed=seed)
    A.enable_cost_schedule(True)
    C.enable_cost_schedule(True)
    ta, tc = A.reset(), C.reset()
    P = A.compiled.program
    rs = np.random.RandomState(seed)
    K, T = 3, 4
    firsts = 0
    for i in range(steps):
        if i in forced:
            A.state_i32[::2, A.layout.o_reset_next] = 1
            C.state_i32[::2, C.layout.o_reset_next] = 1
        torch.cuda.synchronize()
        kept = [t.clone() for t in (A.state_f64, A.state_i32, A._cost, A.repeat_count, ta.reward, ta.discount, ta.step_type,
                                    ta.observation['image'])]
        last = getattr(A, '_last_action', None)
        A.rollout_candidates(draw_candidates(P, n, K, T, rs, name))
        torch.cuda.synchronize()
        now = (A.state_f64, A.state_i32, A._cost, A.repeat_count, ta.reward, ta.discount, ta.step_type, ta.observation['image'])
        for j, (x, y) in enumerate(zip(kept, now)):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (i, j)
        assert getattr(A, '_last_action', None) is last and A.action_repeat == 1
        a = draw_actions(P, n, rs)
        ta, tc = A.step(a), C.step(a)
        torch.cuda.synchronize()
        assert torch.equal(A.state_i32, C.state_i32) and torch.equal(b64(A.state_f64), b64(C.state_f64)), i
        assert torch.equal(ta.step_type, tc.step_type) and torch.equal(ta.observation['image'], tc.observation['image']), i
        assert torch.equal(b64(ta.reward), b64(tc.reward)) and torch.equal(A.repeat_count, C.repeat_count), i
        firsts += int((ta.step_type == 0).sum())
    assert firsts > 0, 'no episode was opened during the run'
    assert A.reset_pool['on'] == C.reset_pool['on'] and A.kernel_variant == C.kernel_variant
    if name == 'parallelogram_catch':
        assert A.kernel_variant[1], 'not a late-reset program'
    if name == 'red_green_l1':
        assert A.reset_pool['on'], 'not a pool program'
    A.raise_faults()
    A.close()
    C.close()


# -- 4. trajectories --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,seed', [('colliding_predators', 7), ('cleanup', 7)])
def test_candidate_trajectories(name, seed):
    """record=key and record=[two keys], a float32 and a float16 table: every [k] block equals the witness rollout's
    trajectory; a call without record made afterwards writes nothing to the earlier tensors."""
    import torch
    from test_rollout_trajectory_gpu import two_tables, same
    from test_sprite_table_gpu import _env
    tables = two_tables(name)
    n, K, T = 5, 3, 5
    A = _env(name, n, tables, seed=seed)
    B = _env(name, n, tables, seed=seed, reset_pool=False)
    A.reset()
    B.reset()
    rs = np.random.RandomState(seed)
    P = A.compiled.program
    for _ in range(3):
        a = draw_actions(P, n, rs)
        A.step(a)
        B.step(a)
    for record in ('full', 'h', ['h', 'full']):
        acts = draw_candidates(P, n, K, T, rs)
        want = witness(B, acts, record=record)
        got = A.rollout_candidates(acts, record=record)
        torch.cuda.synchronize()
        assert len(got) == 4 and sorted(got[3]) == sorted([record] if isinstance(record, str) else record)
        assert_same(got, want, (name, record))
        for key, t in got[3].items():
            assert tuple(t.shape) == (K, T, n) + tuple(A.tables[key].shape[1:])
            assert same(t, want[3][key]), (record, key)
        assert torch.equal(A.state_i32, B.state_i32) and torch.equal(b64(A.state_f64), b64(B.state_f64)), record
    assert bool((got[3]['full'][..., 0] == 1).any())   # (live rows: not a comparison of zeros)
    kept = {key: t.clone() for key, t in got[3].items()}
    tabs = {key: t.clone() for key, t in A.tables.items()}
    A.rollout_candidates(draw_candidates(P, n, K, T, rs))
    A.rollout(draw_candidates(P, n, 1, T, rs)[0])
    torch.cuda.synchronize()
    for key in kept:
        assert same(kept[key], got[3][key]), key
    del tabs
    A.close()
    B.close()


# -- 5. sub-batches -----------------------------------------------------------------------------------------------------------
def test_sub_batches_plan_like_one_batch():
    import torch
    from moog import environment, observers
    from moog_demos import example_configs
    n, G, K, T = 12, 2, 3, 5

    def cfg():
        c = example_configs.load('chase_avoid_torus')
        c['observers'] = dict(c['observers'], t=observers.SpriteTable())
        return c

    one = environment.BatchedEnvironment(num_envs=n, seed=13, **cfg())
    sub = environment.SubBatchedEnvironment(num_envs=n, sub_batches=G, seed=13, **cfg())
    one.reset()
    sub.reset()
    rs = np.random.RandomState(2)
    for i in range(6):
        acts = torch.as_tensor(rs.uniform(-1, 1, size=(K, T, n, 2)), device='cuda')
        r1, c1, e1, t1 = one.rollout_candidates(acts, record='t')
        r2, c2, e2, t2 = sub.rollout_candidates(acts, record='t')
        torch.cuda.synchronize()
        assert torch.equal(b64(r1), b64(r2)) and torch.equal(c1, c2) and torch.equal(e1, e2), i
        assert torch.equal(t1['t'].view(torch.int32), t2['t'].view(torch.int32)), i
        a = rs.uniform(-1, 1, size=(n, 2))
        one.step(a)
        sub.step(a)
        assert torch.equal(one.state_i32, sub.state_i32) and torch.equal(b64(one.state_f64), b64(sub.state_f64)), i
    one.close()
    sub.close()


# -- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_env_stepping():
    import torch
    from moog import environment, observers
    from moog_demos import example_configs
    from test_action_repeat import _meta_config
    n = 4
    rs = np.random.RandomState(0)
    cfg = example_configs.load('pong')
    cfg['observers'] = dict(cfg['observers'], t=observers.SpriteTable(), state=observers.RawState())
    env = environment.BatchedEnvironment(num_envs=n, seed=1, **cfg)
    env.reset()
    step = lambda: env.step(rs.uniform(-1, 1, size=(n, 2)))   # noqa: E731
    for shape in ((2, 3, n, 3), (2, 3, n + 1, 2), (2, 3, n), (3, n, 2), (n, 2)):
        with pytest.raises(ValueError, match=r'\[K, T, 4, 2\]|leading \[K, T'):
            env.rollout_candidates(np.zeros(shape))
        step()
    for K in (0, _abi.MOOG_MAX_PLAN_CANDIDATES + 1):
        with pytest.raises(ValueError, match='1 .. %d' % _abi.MOOG_MAX_PLAN_CANDIDATES):
            env.rollout_candidates(np.zeros((K, 2, n, 2)))
        step()
    for T in (0, _abi.MOOG_MAX_ACTION_REPEAT + 1):
        with pytest.raises(ValueError, match='1 .. %d' % _abi.MOOG_MAX_ACTION_REPEAT):
            env.rollout_candidates(np.zeros((2, T, n, 2)))
        step()
    ok = np.zeros((2, 3, n, 2))
    with pytest.raises(KeyError, match='nope'):
        env.rollout_candidates(ok, record='nope')
    for key in ('image', 'state'):
        with pytest.raises(TypeError, match='SpriteTable'):
            env.rollout_candidates(ok, record=key)
    with pytest.raises(ValueError, match='twice'):
        env.rollout_candidates(ok, record=['t', 't'])
    step()
    env.set_action_repeat(2)
    with pytest.raises(NotImplementedError, match='action_repeat=2'):
        env.rollout_candidates(ok)
    step()
    assert bool((env.repeat_count == 2).all())
    env.set_action_repeat(1)
    rewards, count, ended = env.rollout_candidates(rs.uniform(-1, 1, size=(2, 3, n, 2)))
    assert rewards.shape == (2, 3, n) and bool((count > 0).all())
    # the C entry point refuses what the Python layer would never hand it, and launches nothing
    import ctypes
    lib, buf = env._lib, torch.zeros(64, dtype=torch.float64, device='cuda')
    p = ctypes.c_void_p(buf.data_ptr())
    call = lambda K, T, a=p, r=p, c=p, d=p: lib.moog_engine_plan_sequences(env._handle, a, K, T, 48, 16, r, 12, 4, c, d, 4, None, None)   # noqa: E731
    assert call(0, 2) == _abi.MOOG_E_INVALID and call(_abi.MOOG_MAX_PLAN_CANDIDATES + 1, 2) == _abi.MOOG_E_INVALID
    assert call(2, 0) == _abi.MOOG_E_INVALID and call(2, _abi.MOOG_MAX_ACTION_REPEAT + 1) == _abi.MOOG_E_INVALID
    assert call(2, 2, a=None) == _abi.MOOG_E_INVALID and call(2, 2, r=None) == _abi.MOOG_E_INVALID
    assert call(2, 2, c=None) == _abi.MOOG_E_INVALID and call(2, 2, d=None) == _abi.MOOG_E_INVALID
    step()
    env.close()

    meta = environment.BatchedEnvironment(num_envs=n, seed=1, **_meta_config())
    meta.reset()
    with pytest.raises(NotImplementedError, match='host-side meta-state rules'):
        meta.rollout_candidates(ok)
    meta.step(rs.uniform(-1, 1, size=(n, 2)))
    meta.close()

    auto = environment.BatchedEnvironment(num_envs=n, seed=1, layer_capacity='auto', **example_configs.load('cleanup'))
    auto.reset()
    k = len(auto.action_space.action_keys)
    with pytest.raises(NotImplementedError, match="layer_capacity='auto'"):
        auto.rollout_candidates(np.zeros((2, 3, n, k, 2)))
    auto.step(rs.uniform(-1, 1, size=(n, k, 2)))
    auto.close()
