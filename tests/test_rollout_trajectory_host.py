"""Rollout trajectories, what needs no device: the entry point moog_engine_set_table_trajectory in the header, the binding and
the built library; the version numbers and program bytes it leaves alone; the refusals rollout(record=...) gives before it
touches an engine."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import helpers
from moog import _abi, _engine, environment, observers
from test_action_repeat import _meta_config
from test_rollout_host import _engineless


def test_abi_declares_the_trajectory_call_and_leaves_the_programs_alone():
    assert 'moog_engine_set_table_trajectory' in _engine.SYMBOLS
    hdr = open(_abi.HEADER).read()
    assert 'moog_engine_set_table_trajectory' in set(re.findall(r'\b(moog_\w+)\s*\(', hdr))
    lib = _engine.load_library()
    assert hasattr(lib, 'moog_engine_set_table_trajectory')
    # (a null engine is refused, not dereferenced -- whatever else the call is handed)
    buf = (ctypes.c_float * 8)()
    assert lib.moog_engine_set_table_trajectory(None, 0, ctypes.addressof(buf), 8) == _abi.MOOG_E_INVALID
    assert b'null engine' in lib.moog_last_error()
    assert lib.moog_engine_set_table_trajectory(None, -1, None, 0) == _abi.MOOG_E_INVALID
    assert _abi.MOOG_ABI_VERSION == 31 and _abi.MOOG_PROGRAM_VERSION == 30 and _abi.MOOG_K_COUNT == 5
    assert lib.moog_abi_version() == 31
    P = helpers.compiled('colliding_predators_32').program
    assert P.abi_version == _abi.MOOG_PROGRAM_VERSION
    h = ctypes.c_uint64()
    _engine.check(lib, lib.moog_program_step_kernel(ctypes.byref(P), None, None, ctypes.byref(h)))
    assert '%016x' % h.value == '417c47560f31861d'   # (the headline's specialised kernel keeps its name)


def _with_tables(name='pong'):
    from moog_demos import example_configs
    cfg = example_configs.load(name)
    cfg['observers'] = dict(cfg['observers'], t=observers.SpriteTable(), h=observers.SpriteTable(dtype='float16'),
                            state=observers.RawState())
    env = _engineless(**cfg)
    env.observers = cfg['observers']   # (what __init__ keeps of the config: the refusals read nothing else)
    return env


def test_record_refusals_need_no_device():
    """A key that is no observer of the config, a key of an observer that is no SpriteTable, a repeated key and an empty list
    are refused by name before anything touches a device -- whatever the actions are."""
    seq = np.zeros((3, 4, 2))
    env = _with_tables()
    with pytest.raises(KeyError, match='nope'):
        env.rollout(seq, record='nope')
    with pytest.raises(KeyError, match='nope'):
        env.rollout(seq, record=['t', 'nope'])
    for key in ('image', 'state'):
        with pytest.raises(TypeError, match='SpriteTable'):
            env.rollout(seq, record=key)
    with pytest.raises(TypeError, match='PILRenderer'):
        env.rollout(seq, record=('t', 'image'))
    with pytest.raises(ValueError, match='twice'):
        env.rollout(seq, record=['t', 'h', 't'])
    for empty in ([], ()):
        with pytest.raises(ValueError, match='empty'):
            env.rollout(seq, record=empty)
    # everything _check_rollout refuses stays refused, with a good record too
    for T in (0, _abi.MOOG_MAX_ACTION_REPEAT + 1):
        with pytest.raises(ValueError, match='1 .. %d' % _abi.MOOG_MAX_ACTION_REPEAT):
            env.rollout(np.zeros((T, 4, 2)), record='t')
    env._action_repeat = 2
    with pytest.raises(NotImplementedError, match='action_repeat=2'):
        env.rollout(seq, record=['t', 'h'])


def test_rollout_without_record_refuses_what_it_refused():
    seq = np.zeros((3, 4, 2))
    with pytest.raises(NotImplementedError, match='host-side meta-state rules'):
        _engineless(**_meta_config()).rollout(seq, record=None)
    with pytest.raises(NotImplementedError, match='host-side meta-state rules'):
        _engineless(**_meta_config()).rollout(seq)


def test_both_rollouts_take_record():
    for cls in (environment.BatchedEnvironment, environment.SubBatchedEnvironment):
        p = inspect.signature(cls.rollout).parameters
        assert list(p) == ['self', 'actions', 'record'] and p['record'].default is None, cls
    p = inspect.signature(environment.BatchedEnvironment._rollout_packed).parameters
    assert list(p) == ['self', 'a', 'rewards', 'traj'] and p['traj'].default is None
    from moog import sharding
    assert not hasattr(sharding.MultiDeviceEnvironment, 'rollout')   # (has none, and gets none here)


def test_all_three_kernels_of_the_headline_object_keep_small_frames(tmp_path):
    """A specialised object is linked from one unit per kernel (csrc/moog_step_spec.hip), so its .hip_fatbin section holds
    three bundles, and test_host.py::test_kernel_scratch_report reads the first.  Here every bundle is read: the one-step,
    the repeat and the recording kernel of the headline's object are all there and keep that test's bounds (<= 128 B of
    scratch, <= 40 spilled VGPRs); the one-step kernel spills nothing."""
    import glob
    import os
    import subprocess
    from moog import _spec
    llvm = '/opt/rocm/lib/llvm/bin'
    objs = glob.glob(os.path.join(_spec.SPEC_DIR, 'step_417c47560f31861d_*.so'))
    if not objs or not os.path.exists(os.path.join(llvm, 'llvm-readelf')):
        pytest.skip('no built specialised object / no llvm tools here')
    fat = str(tmp_path / 'fat.bin')
    subprocess.check_call([os.path.join(llvm, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, objs[0], str(tmp_path / 'scratch.o')])
    data, magic = open(fat, 'rb').read(), b'__CLANG_OFFLOAD_BUNDLE__'
    starts = [m.start() for m in re.finditer(re.escape(magic), data)]
    assert len(starts) == 3, starts
    rows = {}
    for i, a in enumerate(starts):
        piece, co = str(tmp_path / ('bundle%d.bin' % i)), str(tmp_path / ('dev%d.co' % i))
        with open(piece, 'wb') as f:
            f.write(data[a:starts[i + 1] if i + 1 < len(starts) else len(data)])
        subprocess.check_call([os.path.join(llvm, 'clang-offload-bundler'), '--unbundle', '--type=o',
                               '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + piece, '--output=' + co])
        notes = subprocess.check_output([os.path.join(llvm, 'llvm-readelf'), '--notes', co]).decode()
        for block in notes.split('  - .agpr_count')[1:]:
            g = lambda k: int(re.search(r'\.' + k + r':\s+(\d+)', block).group(1))   # noqa: E731
            rows[re.search(r'\.name:\s+(\S+)', block).group(1)] = (g('private_segment_fixed_size'), g('vgpr_spill_count'))
    print(rows)
    kinds = {'Lb0ELb0E': 'one step', 'Lb1ELb0E': 'repeat', 'Lb1ELb1E': 'record'}
    assert len(rows) == 3 and all(sum(k in name for name in rows) == 1 for k in kinds), rows
    for name, (scratch, spilled) in rows.items():
        assert 'step_kernel' in name and scratch <= 128 and spilled <= 40, (name, scratch, spilled)
        if 'Lb0ELb0E' in name:
            assert (scratch, spilled) == (0, 0), (name, scratch, spilled)
