"""Rollout trajectories on the MI355X (BatchedEnvironment.rollout(record=...), include/moog_engine.h
moog_engine_set_table_trajectory): the SpriteTables of every env-step of a rollout, written by the step launch itself.

Witnesses: the engine's own single-step path (trajectory[key][t] is, bit for bit, tables[key] after the t-th step() call of a
twin engine), the CPU oracle's record after every env-step (episode ends and the three reset paths), a single batch against
sub-batches, and guard patterns around the recorded slices."""
import numpy as np
import pytest

import helpers
import test_rollout_gpu as ro
import test_sprite_table_host as host
from moog import _abi, observers
from test_sprite_table_gpu import _env

pytestmark = pytest.mark.gpu
ALL = observers.SpriteTable.ALL_COLUMNS
INTEGER_COLUMNS = ('alive', 'layer', 'opacity', 'shape_id', 'n_vertices')


def two_tables(name):
    """'full': float32, every column (the default ones where the program keeps no scale / aspect_ratio); 'h': float16, three
    columns with `alive` and a colour, over a subset of the layers whose row count is odd where the layers allow."""
    c = helpers.compiled(name)
    cols = ALL if c.program.sprite_factors else observers.SpriteTable.DEFAULT_COLUMNS
    layers = list(c.layer_slots)
    rows = lambda ks: sum(c.layer_slots[k][1] for k in ks)   # noqa: E731
    pairs = [(a, b) for a, b in zip(layers, layers[1:]) if rows((a, b)) % 2 == 1]
    odd = [(k,) for k in layers if rows((k,)) % 2 == 1]
    subset = (pairs + odd + [tuple(layers[:1])])[0]
    return {'full': observers.SpriteTable(columns=cols), 'h': observers.SpriteTable(layers=subset, columns=('alive', 'c2', 'x'), dtype='float16')}


def bits(t):
    import torch
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def same(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# -- 1. bit for bit against single calls ------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 3, 8])
@pytest.mark.parametrize('name,seed,kernel,f32', ro.EQUAL_CASES)
def test_trajectory_equals_single_calls_bit_for_bit(name, seed, kernel, f32, T):
    """Two engines, same seed, the quiet windows of test_rollout_gpu.EQUAL_CASES: A rolls out T actions per macro-step and
    records two tables, B makes T single step() calls.  trajectory[key][t] equals B's table after its t-th call as raw bits;
    after the macro-step both state tensors, the rewards and the frame are equal: recording does not perturb the step."""
    import torch
    tables = two_tables(name)
    acts = ro.equal_actions(name, seed, T, f32)
    A = _env(name, ro.EQUAL_N, tables, seed=seed)
    B = _env(name, ro.EQUAL_N, tables, seed=seed)
    if kernel is not None:
        assert A.step_kernel() == kernel and B.step_kernel() == kernel
    shape = {k: tuple(A.tables[k].shape[1:]) for k in tables}
    print(name, 'rows x columns', shape)
    if shape['h'][0] % 2 == 0:
        print(name, ': no subset of layers has an odd row count')
    A.reset()
    B.reset()
    b64 = lambda t: t.view(torch.int64)   # noqa: E731
    for i in range(ro.EQUAL_MACRO):
        seq = acts[i * T:(i + 1) * T]
        ta, rewards, count, traj = A.rollout(seq, record=list(tables))
        assert sorted(traj) == sorted(tables)
        for key in tables:
            assert tuple(traj[key].shape) == (T, ro.EQUAL_N) + shape[key] and traj[key].dtype == A.tables[key].dtype
            assert shape[key] == (len(A.table_rows(key)), len(A.table_columns(key)))
        for t in range(T):
            tb = B.step(seq[t])
            assert torch.equal(b64(rewards[t]), b64(tb.reward)), (i, t)
            for key in tables:
                assert same(traj[key][t], tb.observation[key]), (i, t, key, int((bits(traj[key][t]) != bits(tb.observation[key])).sum()))
        assert bool((count == T).all()), i
        for key in tables:   # (the last step taken is what the table itself shows after the call)
            assert same(traj[key][T - 1], A.tables[key]), (i, key)
        assert torch.equal(A.state_i32, B.state_i32), i
        assert torch.equal(b64(A.state_f64), b64(B.state_f64)), i
        assert torch.equal(ta.step_type, tb.step_type) and torch.equal(b64(ta.discount), b64(tb.discount)), i
        assert torch.equal(ta.observation['image'], tb.observation['image']), i
    assert bool((traj['full'][:, :, :, 0] == 1).any())   # (live rows: not a comparison of zeros)
    A.close()
    B.close()


# -- 2. episode ends, the three reset paths, the oracle ------------------------------------------------------------------
class LoggingOracle(helpers.OracleEnv):
    """An oracle that keeps its record after every step (what expected_run's one-env oracles see of a call)."""
    def step(self, actions, uniforms=None, render=True):
        super().step(actions, uniforms, render)
        if not hasattr(self, 'log'):
            self.log = []
        self.log.append((self.f64.copy(), self.i32.copy(), int(self.step_type[0])))


class Recording(object):
    """What expected_run asks of an env, with every rollout recorded."""
    def __init__(self, env, keys):
        self.env, self.keys, self.traj = env, keys, None
        self.compiled, self.state_i32 = env.compiled, env.state_i32

    def reset(self):
        return self.env.reset()

    def rollout(self, seq):
        ts, rewards, count, self.traj = self.env.rollout(seq, record=self.keys)
        return ts, rewards, count


def table_of(c, T, columns, f, q, shift=0.0):
    """The table T (columns by name) of the records f [n, f64_per_env] / q [n, i32_per_env], cast by numpy, the float
    values moved by `shift` first (test_sprite_table_gpu.expected, over records instead of an engine's tensors)."""
    P, L, S = c.program, c.layout, c.layout.S
    two = lambda o, k: f[:, o:o + 2 * S].reshape(-1, S, 2)[:, :, k]   # noqa: E731
    col3 = lambda k: f[:, L.o_color:L.o_color + 3 * S].reshape(-1, S, 3)[:, :, k]   # noqa: E731
    one = lambda o: f[:, o:o + S]   # noqa: E731
    alive = (q[:, L.o_flags:L.o_flags + S] & _abi.MOOG_F_ALIVE) != 0
    src = {'x': lambda: two(L.o_pos, 0), 'y': lambda: two(L.o_pos, 1), 'x_vel': lambda: two(L.o_vel, 0),
           'y_vel': lambda: two(L.o_vel, 1), 'angle': lambda: one(L.o_angle), 'angle_vel': lambda: one(L.o_angvel),
           'mass': lambda: one(L.o_mass), 'c0': lambda: col3(0), 'c1': lambda: col3(1), 'c2': lambda: col3(2),
           'scale': lambda: one(L.o_scale), 'aspect_ratio': lambda: one(L.o_aspect),
           'opacity': lambda: q[:, L.o_opacity:L.o_opacity + S], 'shape_id': lambda: q[:, L.o_shape:L.o_shape + S],
           'n_vertices': lambda: q[:, L.o_nverts:L.o_nverts + S], 'alive': lambda: alive,
           'layer': lambda: np.broadcast_to(np.array([P.slot_layer[s] for s in range(S)]), alive.shape)}
    slots = [T.row_slot[r] for r in range(T.n_rows)]
    dt = host.sprite_table.table_dtype(T)
    out = np.zeros((f.shape[0], T.n_rows, T.n_cols), dt)
    with np.errstate(all='ignore'):
        for k, name in enumerate(columns):
            v = np.asarray(src[name]())[:, slots]
            if name not in INTEGER_COLUMNS:
                v = v + shift
            out[:, :, k] = np.where(alive[:, slots], v.astype(dt), dt.type(0))
    return out


RECORD_TOL = 1e-9   # what test_rollout_vs_oracle allows between the engine's float record and the oracle's


@pytest.mark.parametrize('T', ro.TS)
@pytest.mark.parametrize('name,n,seed,calls,natural', ro.ORACLE_CASES)
def test_trajectory_with_episode_ends_vs_oracle(name, n, seed, calls, natural, T, monkeypatch):
    """The runs of test_rollout_vs_oracle (episodes ending inside a window, envs that start a call with reset_next set by the
    task or by hand; reset in place, from the pool, by the late-reset kernel), every call recorded.  Exact: the blocks of the
    steps an env did not take are zero bits; the block of its last step equals its table after the call.  Against the oracle's
    record after every env-step: the integer-valued columns exactly numpy's cast, the others within the cast of the record
    moved by -/+ 1e-9 -- the record's tolerance in that test, carried through the (monotonic) cast."""
    import torch
    from test_gpu_parity import download
    monkeypatch.setattr(helpers, 'OracleEnv', LoggingOracle)
    tables = two_tables(name)
    env = _env(name, n, tables, seed=seed)
    rec = Recording(env, list(tables))
    c = env.compiled
    lowered = dict(c.tables)
    seen = {'zero': 0, 'taken': 0}

    def check(call, oracles, want, got):
        f, q = download(env)
        if want is not None:
            m = np.array([w[3] for w in want])
            assert np.array_equal(got[2].cpu().numpy(), m), (call, m)
            for key in tables:
                g = rec.traj[key].cpu().numpy()
                own = env.tables[key].cpu().numpy()
                assert g.shape == (T, n) + own.shape[1:]
                cols = env.table_columns(key)
                integer = np.array([k in INTEGER_COLUMNS for k in cols])
                for i, o in enumerate(oracles):
                    assert not host.bits(g[m[i]:, i]).any(), (call, key, i, 'steps not taken are not zero bits')
                    seen['zero'] += T - m[i]
                    if m[i] >= 1:
                        assert host.same_bits(g[m[i] - 1, i], own[i]), (call, key, i, 'the last step is not the table after the call')
                    log = [r for r in o.log if r[2] != 0]
                    assert len(log) == m[i], (call, i, len(log), m[i])
                    if not log:
                        continue
                    of, oq = np.concatenate([r[0] for r in log]), np.concatenate([r[1] for r in log])   # [m, ...]: one row per step
                    mid, lo, hi = (table_of(c, lowered[key], cols, of, oq, d) for d in (0.0, -RECORD_TOL, RECORD_TOL))
                    x = g[:m[i], i]
                    assert host.same_bits(x[:, :, integer], mid[:, :, integer]), (call, key, i)
                    with np.errstate(invalid='ignore'):
                        inside = ((x >= lo) & (x <= hi)) | (host.bits(x) == host.bits(mid))
                    assert inside.all(), (call, key, i, np.argwhere(~inside)[:4], x[~inside][:4], mid[~inside][:4])
                    seen['taken'] += int(m[i])
            if call == ro.FORCED:
                assert (m[1::4] == 0).all()
        for i, o in enumerate(oracles):   # lock step, as test_rollout_vs_oracle; the next call's log starts empty
            o.f64[0], o.i32[0] = f[i], q[i]
            o.log = []

    inside, starts = ro.expected_run(name, n, seed, T, calls, env=rec, check=check)
    torch.cuda.synchronize()
    env.close()
    assert seen['zero'] > 0 and seen['taken'] > 0
    if natural:
        assert inside > 0 and starts > 0, (inside, starts)


# -- 3. sub-batches --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('G', [2, 3])
def test_sub_batches_record_like_one_batch(G):
    """6 envs as G sub-batches (parts of 3 and of 2 envs) against one batch: trajectory, rewards and count bit for bit.  The
    float16 table has an odd rows x columns, so a part's slice of it starts on an odd half-word."""
    import torch
    name, n, T, seed = 'chase_avoid_torus', 6, 5, 3
    c = helpers.compiled(name)
    layers = list(c.layer_slots)
    odd = [k for k in layers if c.layer_slots[k][1] % 2 == 1]
    tables = {'full': observers.SpriteTable(), 'h': observers.SpriteTable(layers=(odd[0],), columns=('alive', 'c0', 'y'), dtype='float16')}
    one = _env(name, n, tables, seed=seed)
    sub = _env(name, n, tables, seed=seed, sub_batches=G)
    per_env = sub.tables['h'].shape[1] * sub.tables['h'].shape[2]
    assert per_env % 2 == 1   # (G = 2: parts of 3 envs, the second part's slice starts in the middle of a dword)
    one.reset()
    sub.reset()
    rs = np.random.RandomState(seed)
    short = 0
    for i in range(16):
        a = torch.as_tensor(rs.uniform(-1, 1, size=(T, n, 2)), device='cuda')
        (t1, r1, c1, j1), (t2, r2, c2, j2) = one.rollout(a, record=('full', 'h')), sub.rollout(a, record=('full', 'h'))
        torch.cuda.synchronize()
        assert torch.equal(c1, c2) and torch.equal(r1.view(torch.int64), r2.view(torch.int64)), i
        short += int(((c1 > 0) & (c1 < T)).sum())
        for key in tables:
            assert tuple(j2[key].shape) == (T, n) + tuple(sub.tables[key].shape[1:]) and j2[key].is_contiguous()
            assert same(j1[key], j2[key]), (i, key)
        assert torch.equal(one.state_i32, sub.state_i32), i
    assert short > 0, 'no episode ended inside a window'
    one.close()
    sub.close()


# -- 4. nothing outside the buffer, nothing after the call --------------------------------------------------------------------
def test_guards_stay_intact_and_later_calls_write_nothing():
    import torch
    from test_gpu_parity import make_env
    name, seed, n, T = 'colliding_predators', 7, 32, 4
    tables = {'full': observers.SpriteTable(), 'h': observers.SpriteTable(layers=('predators',), columns=('alive', 'c0', 'y'), dtype='float16')}
    acts = ro.equal_actions(name, seed, 8, False)   # (32 env-steps without an episode end: ro.window_is_quiet)
    env, twin = _env(name, n, tables, seed=seed), _env(name, n, tables, seed=seed)
    env.reset()
    twin.reset()
    # slices from the middle of larger tensors, in the step and in the env dimension
    a = env._pack_sequence(acts[:T])
    rewards = torch.empty((T, n), dtype=torch.float64, device=env.device)
    big, cut = {}, {}
    for key in tables:
        rows, cols = env.tables[key].shape[1:]
        guard = 0x7b7b if key == 'h' else 0x7b7b7b7b
        big[key] = torch.full((T + 3, n + 5, rows, cols), guard, dtype=torch.int16 if key == 'h' else torch.int32,
                              device=env.device).view(env.tables[key].dtype)
        cut[key] = big[key][2:2 + T, 3:3 + n]
    assert (cut['h'].data_ptr() - big['h'].data_ptr()) // 2 % 2 == 1   # (the float16 slice starts on an odd half-word)
    env._rollout_packed(a, rewards, cut)
    ta, r2, count, traj = twin.rollout(acts[:T], record=list(tables))
    torch.cuda.synchronize()
    for key in tables:
        assert same(cut[key].contiguous(), traj[key]), key
        outside = torch.ones(big[key].shape, dtype=torch.bool, device=env.device)
        outside[2:2 + T, 3:3 + n] = False
        guard = 0x7b7b if key == 'h' else 0x7b7b7b7b
        assert bool((bits(big[key])[outside] == guard).all()), key
    assert torch.equal(rewards.view(torch.int64), r2.view(torch.int64))
    # kept tensors: a rollout without record, a step and a reset write nothing to them
    kept = {key: t.clone() for key, t in traj.items()}
    kept_cut = {key: big[key].clone() for key in tables}
    for e in (env, twin):
        assert e.action_repeat == 1
        _, _, cnt = e.rollout(acts[T:2 * T])
        assert bool((cnt == T).all()) and e.action_repeat == 1
        e.step(acts[2 * T])
        assert bool((e.repeat_count == 1).all())   # (a step() after the call takes ONE env-step)
    assert torch.equal(env.state_i32, twin.state_i32) and torch.equal(env.state_f64.view(torch.int64), twin.state_f64.view(torch.int64))
    env.set_action_repeat(3)
    env.step(acts[2 * T + 1])
    assert bool((env.repeat_count == 3).all())
    for e in (env, twin):
        e.reset()
    torch.cuda.synchronize()
    for key in tables:
        assert same(kept[key], traj[key]), key
        assert same(kept_cut[key], big[key]), key
    plain = make_env(name, n, seed=seed)   # (an engine without tables rolls out as ever, and has nothing to record)
    plain.reset()
    with pytest.raises(KeyError):
        plain.rollout(acts[:T], record='full')
    assert len(plain.rollout(acts[:T])) == 3
    for e in (env, twin, plain):
        e.close()


# -- 5. colours written inside the window ------------------------------------------------------------------------------------
def test_colours_written_inside_the_window_show():
    """lambda_zoo: its first rule (ModifySprites over the fountains, sample_one) sets the c2 of one fountain that is below the
    threshold in every env-step from the first one on, through the modifier's COL_SET on the step path; its only task that
    ends an episode is the timeout of 14 steps, so the 8 env-steps after a reset are a quiet window."""
    import torch
    name, n, T, seed = 'lambda_zoo', 8, 8, 2
    tables = {'col': observers.SpriteTable(columns=('c0', 'c1', 'c2', 'opacity')),
              'col16': observers.SpriteTable(layers=('fountains',), columns=('c2', 'opacity', 'alive'), dtype='float16')}
    A, B = _env(name, n, tables, seed=seed), _env(name, n, tables, seed=seed)
    A.reset()
    B.reset()
    acts = np.random.RandomState(seed).uniform(-1, 1, size=(T, n, 2))
    ta, rewards, count, traj = A.rollout(acts, record=('col', 'col16'))
    assert bool((count == T).all())
    for t in range(T):
        tb = B.step(acts[t])
        assert bool((tb.step_type == 1).all())
        for key in tables:
            assert same(traj[key][t], tb.observation[key]), (t, key)
    col = traj['col'].cpu().numpy()
    changed = (host.bits(col[1:]) != host.bits(col[:-1])).any(axis=(0, 2, 3))
    print('envs whose colours change between two steps of the window:', int(changed.sum()), 'of', n)
    assert changed.any(), 'no colour changed inside the window: the test shows nothing'
    assert torch.equal(A.state_f64.view(torch.int64), B.state_f64.view(torch.int64))
    A.close()
    B.close()
