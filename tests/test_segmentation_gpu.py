"""Segmentation observer on the MI355X (include/moog_engine.h moog_engine_add_segmentation): the id images the ids kernel
writes against the masks the reference's own PILRenderer drew (tests/golden/seg_zoo_l*.npz), against the RGB path of the same
engine at batch size, and through sub-batches, facades, layer growth and the launch accounting."""
import os

import numpy as np
import pytest

import helpers
from moog import _abi, _compiler, observers
from moog_demos import example_configs
from moog_demos.example_configs import seg_zoo

pytestmark = pytest.mark.gpu

CAPACITY = {4: {'prey': 8, 'predators': 8}}   # (the capacities level 4 was recorded with: the defaults, spelled out)


def _env(cfg, n, seed=0, sub_batches=None, **kw):
    from moog import environment
    if sub_batches:
        return environment.SubBatchedEnvironment(num_envs=n, sub_batches=sub_batches, seed=seed, **cfg, **kw)
    return environment.BatchedEnvironment(num_envs=n, seed=seed, **cfg, **kw)


def _without(cfg, cls=observers.Segmentation):
    out = dict(cfg)
    out['observers'] = {k: o for k, o in cfg['observers'].items() if not isinstance(o, cls)}
    return out


def _actions(n, calls, seed=5):
    import torch
    g = torch.Generator().manual_seed(seed)
    return [torch.rand((n, 2), generator=g, dtype=torch.float64) * 2 - 1 for _ in range(calls)]


def recording(level):
    with np.load(os.path.join(helpers.GOLDEN, 'seg_zoo_l%d.npz' % level)) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('level', [0, 1, 2, 3, 4])
def test_masks_teacher_forced_vs_reference(level):
    """All recorded calls at once (env i starts from the reference state of call i, with the uniforms that call consumed):
    the mask of call i + 1 equals the reference's in every byte, for every Segmentation key; and the frame equals too."""
    import test_gpu_parity as tgp
    fx = recording(level)
    cfg = seg_zoo.get_config(level)
    cap = CAPACITY.get(level)
    c = _compiler.compile_config(layer_capacity=cap, **cfg)
    T = len(fx['step_type'])
    ts = list(range(1, T))
    env = _env(cfg, len(ts), layer_capacity=cap)
    L = c.layout
    f64 = np.zeros((len(ts), L.f64_per_env))
    i32 = np.zeros((len(ts), L.i32_per_env), np.int32)
    for i, t in enumerate(ts):
        helpers.records_from_fixture(fx, t - 1, c, f64, i32, env=i)
    tgp.upload(env, f64, i32)
    env.check_faults = False
    out = env.step(np.stack([helpers.action_of(fx, t) for t in ts]), injected_uniforms=tgp.padded_uniforms(fx, ts))
    assert np.array_equal(out.step_type.cpu().numpy(), fx['step_type'][1:])
    assert np.array_equal(out.observation['image'].cpu().numpy(), fx['image'][1:])
    for key in seg_zoo.segmentations(level):
        ids = out.observation[key]
        assert ids.dtype == env._torch.uint8 and tuple(ids.shape) == (len(ts),) + fx['ids_' + key].shape[1:]
        bad = np.nonzero((ids.cpu().numpy() != fx['ids_' + key][1:]).reshape(len(ts), -1).any(axis=1))[0]
        assert bad.size == 0, ('%s: masks that differ from the reference\'s' % key, (bad + 1).tolist())
    # call 0 (a reset) from its own state: a render call, records derived from the stored state
    helpers.records_from_fixture(fx, 0, c, f64, i32, env=0)
    tgp.upload(env, f64, i32)
    obs = env.observation()
    for key in seg_zoo.segmentations(level):
        assert np.array_equal(obs[key][0].cpu().numpy(), fx['ids_' + key][0]), key
    env.close()


@pytest.mark.parametrize('size', [(64, 64), (128, 128), (40, 24)])
def test_mask_is_the_red_channel_of_id_coloured_frames(size):
    """seg_zoo level 5: every sprite opaque, sprite k coloured (k + 1, 0, 0), identity colour map, black background -- the
    frame's channel 0 IS the instance mask over all layers.  256 envs, 60 random-action calls across collisions and
    auto-resets, every byte of every call."""
    import torch
    n, calls = 256, 60
    env = _env(seg_zoo.get_config(5, image_size=size), n, seed=3)
    acts = _actions(n, calls)
    ts = env.reset()
    resets = seen = 0
    for t in range(calls + 1):
        frame, mask = ts.observation['image'], ts.observation['seg']
        assert tuple(mask.shape) == (n, size[1], size[0]) and tuple(frame.shape) == (n, size[1], size[0], 3)
        assert torch.equal(frame[..., 0], mask), (size, t, int((frame[..., 0] != mask).sum()))
        assert not bool(frame[..., 1:].any())
        seen = max(seen, int(mask.max()))
        if t == calls:
            break
        ts = env.step(acts[t])
        resets += int((ts.step_type == 0).sum().item())
    assert resets > n and seen == len(env.segmentation_rows('seg')) == 17
    env.close()


def test_result_neutral_and_specialised():
    """Timesteps, frames, tables and records of an env with the observers equal those without them, bit for bit, over 40
    calls; a BASELINE workload keeps its specialised step kernel."""
    import torch
    n, calls = 64, 40
    cfg = seg_zoo.get_config(4)
    cfg['observers'] = dict(cfg['observers'], lay=observers.Segmentation(mode='layer'))
    a, b = _env(cfg, n, seed=2), _env(_without(cfg), n, seed=2)
    acts = _actions(n, calls)
    ta, tb = a.reset(), b.reset()
    for t in range(calls + 1):
        bits = lambda x: x.view(torch.int64)   # (NaN rewards on FIRST timesteps: compared as bit patterns)
        for x, y in ((ta.step_type, tb.step_type), (bits(ta.reward), bits(tb.reward)), (bits(ta.discount), bits(tb.discount)),
                     (ta.observation['image'], tb.observation['image']), (ta.observation['table'], tb.observation['table']),
                     (a.state_i32, b.state_i32), (bits(a.state_f64), bits(b.state_f64))):
            assert torch.equal(x, y), t
        if t < calls:
            ta, tb = a.step(acts[t]), b.step(acts[t])
    assert bool(ta.observation['seg'].any()) and bool(ta.observation['lay'].any())
    a.close()
    b.close()
    cfg = example_configs.load('colliding_predators_32')
    plain = _env(cfg, 32)
    cfg['observers'] = dict(cfg['observers'], seg=observers.Segmentation())
    env = _env(cfg, 32)
    assert plain.step_kernel() == 'specialised' == env.step_kernel()
    ts = env.reset()
    ts = env.step(env.random_action())
    assert bool(ts.observation['seg'].any())
    env.close()
    plain.close()


def test_sub_batches_reset_mask_and_action_repeat():
    import torch
    n = 64
    cfg = seg_zoo.get_config(0)
    whole, parts = _env(cfg, n, seed=4), _env(cfg, n, seed=4, sub_batches=2)
    acts = _actions(n, 8)
    tw, tp = whole.reset(), parts.reset()
    for t in range(8):
        for key in ('seg', 'seg_layer', 'image'):
            assert torch.equal(tw.observation[key], tp.observation[key]), (key, t)
        tw, tp = whole.step(acts[t]), parts.step(acts[t])
    assert parts.segmentation_rows('seg') == whole.segmentation_rows('seg') and tp.observation['seg'].data_ptr() == parts.view_images['seg'].data_ptr()
    parts.close()
    # reset with an env mask: the masked envs show their new episode, the others what they showed
    before = tw.observation['seg'].clone()
    mask = torch.zeros(n, dtype=torch.uint8)
    mask[::2] = 1
    ts = whole.reset(env_mask=mask)
    assert torch.equal(ts.observation['seg'][1::2], before[1::2]) and not torch.equal(ts.observation['seg'][::2], before[::2])
    assert torch.equal(ts.observation['seg'], whole.observation()['seg'])
    # action_repeat = 3: the mask after the call is the mask after three single calls
    single = _env(cfg, n, seed=9)
    triple = _env(cfg, n, seed=9, action_repeat=3)
    single.reset()
    triple.reset()
    act = acts[0]
    for _ in range(3):
        ts1 = single.step(act)
    ts3 = triple.step(act)
    assert torch.equal(ts1.observation['seg'], ts3.observation['seg']) and torch.equal(single.state_i32, triple.state_i32)
    for e in (whole, single, triple):
        e.close()


def test_observation_follows_the_state_tensors():
    """observation() draws the masks from the records as they are: after an edit of the state tensors, after restore()."""
    import torch
    env = _env(seg_zoo.get_config(0), 8, seed=1)
    env.reset()
    first = env.observation()['seg'].clone()
    snap = env.snapshot()
    rows = env.segmentation_rows('seg')
    agent = 1 + rows.index(('agent', 0))
    assert bool((first == agent).any())
    L = env.layout
    slot = env.compiled.layer_slots['agent'][0]
    env.state_i32[:, L.o_opacity + slot] = 0   # the agent turns invisible: it owns no pixel
    hidden = env.observation()['seg']
    assert not bool((hidden == agent).any()) and bool((hidden != first).any())
    env.restore(snap)
    assert torch.equal(env.observation()['seg'], first)
    env.close()


def test_dynamic_layers_ids_are_table_rows_and_fit():
    """seg_zoo level 4: every id v in a mask is a live row v - 1 of the SpriteTable over the same layers; after
    fit_layer_capacity() rows and masks are those of the new capacities, naming the same sprites."""
    import torch
    n = 128
    env = _env(seg_zoo.get_config(4), n, seed=6, layer_capacity={'prey': 12, 'predators': 12})
    assert env.segmentation_rows('seg') == env.table_rows('table')
    alive = env.table_columns('table').index('alive')
    ts = env.reset()
    seen = set()
    for t in range(20):
        ts = env.step(env.random_action())
        mask, table = ts.observation['seg'], ts.observation['table']
        present = torch.zeros((n, 256), dtype=torch.bool, device=mask.device)
        present.scatter_(1, mask.reshape(n, -1).long(), True)
        rows = table.shape[1]
        assert not bool(present[:, rows + 1:].any())
        assert bool((table[:, :, alive][present[:, 1:rows + 1]] == 1).all()), t
        seen |= set(torch.unique(mask).tolist())
    assert len(seen) > 6
    rows_before = env.segmentation_rows('seg')
    before = ts.observation['seg'].cpu().numpy()
    caps = env.fit_layer_capacity()
    assert caps and all(v < 12 for v in caps.values())
    rows_after = env.segmentation_rows('seg')
    fresh = _compiler.compile_config(layer_capacity=dict({'prey': 12, 'predators': 12}, **caps), **seg_zoo.get_config(4))
    assert rows_after == fresh.segmentation_rows['seg'] == env.table_rows('table') and rows_after != rows_before
    after = env._observation()['seg'].cpu().numpy()   # (refilled at once, like the tables)
    decode = lambda m, rows: np.array([-1] + [rows_before.index(r) if r in rows_before else -2 for r in rows])[m]
    assert np.array_equal(decode(before, rows_before), decode(after, rows_after))
    assert np.array_equal(env.observation()['seg'].cpu().numpy(), after)
    env.close()


def test_facades_carry_the_entry():
    from moog import environment
    from moog.env_wrappers import gym_wrapper
    cfg = seg_zoo.get_config(1)
    env = environment.Environment(**cfg)
    ts = env.reset()
    assert list(ts.observation) == ['image', 'seg'] and ts.observation['seg'].shape == (24, 40) and ts.observation['seg'].dtype == np.uint8
    ts = env.step(np.zeros(2))
    assert ts.observation['seg'].shape == (24, 40) and ts.observation['seg'].any()
    spec = env.observation_spec()
    assert spec['seg'].shape == (24, 40) and spec['seg'].dtype == np.uint8
    g = gym_wrapper.GymWrapper(environment.Environment(**seg_zoo.get_config(1)))
    assert set(g.observation_space.spaces) == {'image', 'seg'} and g.observation_space.spaces['seg'].shape == (24, 40)
    obs = g.reset()
    assert obs['seg'].shape == (24, 40)
    env.close()


def test_launch_accounting_and_refusals_of_the_engine():
    """With timing on, MOOG_K_VIEWS counts one bracket per call for the segmentations (their derive launch, raster launches
    and crop together); with the buffers unbound it counts none.  The engine's own refusals say why."""
    import ctypes
    from moog import _engine
    env = _env(seg_zoo.get_config(0), 16)
    env.set_timing(True)
    env.reset()
    for _ in range(4):
        env.step(env.random_action())
    env.observation()
    env._torch.cuda.synchronize()
    assert env.kernel_time(_abi.MOOG_K_VIEWS)[1] == 6 and env.kernel_time(_abi.MOOG_K_RASTER)[1] == 6
    lib, h = env._lib, env._handle
    for idx in env._segmentation_index.values():
        _engine.check(lib, lib.moog_engine_set_segmentation_image(h, idx, None))
    kept = {k: env.view_images[k].clone() for k in env._segmentation_index}
    for _ in range(3):
        env.step(env.random_action())
    env._torch.cuda.synchronize()
    assert env.kernel_time(_abi.MOOG_K_VIEWS)[1] == 0 and env.kernel_time(_abi.MOOG_K_RASTER)[1] == 3   # (a read clears the counts)
    assert all(env._torch.equal(env.view_images[k], v) for k, v in kept.items())
    G = _abi.Segmentation()
    G.width, G.height, G.n_slots = 64, 64, env.compiled.program.n_slots
    idx = ctypes.c_int32()
    assert lib.moog_engine_add_segmentation(h, ctypes.byref(G), ctypes.byref(idx)) != 0   # a third
    assert b'MOOG_MAX_SEGMENTATIONS' in lib.moog_last_error()
    env.close()
    env = _env(_without(seg_zoo.get_config(0)), 4)
    lib, h = env._lib, env._handle
    for w, hgt, slots, why in ((129, 64, env.compiled.program.n_slots, b'span rasteriser'), (64, 0, env.compiled.program.n_slots, b'span rasteriser'),
                               (64, 64, 3, b'n_slots')):
        G.width, G.height, G.n_slots = w, hgt, slots
        assert lib.moog_engine_add_segmentation(h, ctypes.byref(G), ctypes.byref(idx)) != 0 and why in lib.moog_last_error()
    assert lib.moog_engine_set_segmentation_image(h, 0, None) != 0
    env.close()
