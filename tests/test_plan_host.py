"""Candidate rollouts, what needs no device: the entry point moog_engine_plan_sequences in the header, the binding and the
built library; the version numbers it leaves alone; the six candidate units of the step kernel and their frames; the
refusals rollout_candidates() gives before it touches an engine."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest

import helpers
from moog import _abi, _digest, _engine, environment
from test_action_repeat import _meta_config
from test_host import PKG, _kernel_notes
from test_rollout_host import _engineless

TAGS = ('f3', 'f4', 't3', 't4', 'm3', 'm4')


def test_abi_declares_the_plan_call_and_leaves_the_versions_alone():
    for name in ('moog_engine_plan_sequences', 'moog_engine_plan_kernel'):
        assert name in _engine.SYMBOLS
        assert name in set(re.findall(r'\b(moog_\w+)\s*\(', open(_abi.HEADER).read()))
        assert hasattr(_engine.load_library(), name)
    lib = _engine.load_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    # (a null engine is refused, not dereferenced -- whatever else the call is handed)
    assert lib.moog_engine_plan_sequences(None, p, 2, 2, 64, 32, p, 8, 4, p, p, 4, None, None) == _abi.MOOG_E_INVALID
    assert lib.moog_engine_plan_sequences(None, None, 0, 0, 0, 0, None, 0, 0, None, None, 0, None, None) == _abi.MOOG_E_INVALID
    assert lib.moog_engine_plan_kernel(None, None) == _abi.MOOG_E_INVALID
    assert 64 <= _abi.MOOG_MAX_PLAN_CANDIDATES <= 65535
    assert _abi.MOOG_ABI_VERSION == 31 and _abi.MOOG_PROGRAM_VERSION == 30 and _abi.MOOG_K_COUNT == 5
    assert lib.moog_abi_version() == 31
    P = helpers.compiled('colliding_predators_32').program
    h = ctypes.c_uint64()
    _engine.check(lib, lib.moog_program_step_kernel(ctypes.byref(P), None, None, ctypes.byref(h)))
    assert '%016x' % h.value == '417c47560f31861d'   # (the headline's specialised kernels keep their name)


def test_the_six_candidate_units_are_built_with_one_step_kernel_each(tmp_path, capsys):
    """lib/moog_step_{f3,f4,t3,t4,m3,m4}rp.o exist, are no older than the digest file of the build that made the library (and
    that library carries the digest of the sources as they are), and each holds exactly one step kernel -- the candidate
    kernel -- whose frame is printed (pytest -s)."""
    if not os.path.exists('/opt/rocm/lib/llvm/bin/llvm-readelf'):
        pytest.skip('no llvm tools here')
    lib_dir = os.path.join(PKG, 'lib')
    assert _digest.digest_of(_engine.LIB_PATH) == _digest.source_digest(), 'libmoog_hip.so is not the build of these sources'
    for tag in TAGS:
        obj = os.path.join(lib_dir, 'moog_step_%srp.o' % tag)
        assert os.path.exists(obj), obj
        assert os.path.getmtime(obj) <= os.path.getmtime(_engine.LIB_PATH), (obj, 'newer than the library: not linked into it')
        kernels = [r for r in _kernel_notes(obj, tmp_path) if 'step_kernel' in r[0]]
        assert len(kernels) == 1 and 'plan_step_kernel' in kernels[0][0], (tag, kernels)
        with capsys.disabled():
            print('moog_step_%srp.o %-60s scratch %5d B  spilled VGPRs %4d  SGPRs %5d  VGPRs %3d' % ((tag,) + kernels[0]))
    assert len(glob.glob(os.path.join(lib_dir, 'moog_step_*rp.o'))) == 6


def test_the_headline_plan_object_keeps_a_small_frame(tmp_path, capsys):
    """The candidate kernel specialised for the headline's program lives in an object of its own beside step_<hash>_*.so
    (that one keeps its three kernels); it carries the build's digest and keeps the bounds test_host.py sets for the
    headline's kernels: <= 128 B of scratch, <= 40 spilled VGPRs."""
    from moog import _spec
    if not os.path.exists('/opt/rocm/lib/llvm/bin/llvm-readelf'):
        pytest.skip('no llvm tools here')
    objs = glob.glob(os.path.join(_spec.SPEC_DIR, 'plan_417c47560f31861d_*.so'))
    assert len(objs) == 1, objs
    assert _spec.is_current(objs[0])
    kernels = [r for r in _kernel_notes(objs[0], tmp_path) if 'step_kernel' in r[0]]
    assert len(kernels) == 1 and 'plan_step_kernel' in kernels[0][0], kernels
    with capsys.disabled():
        print('%s %-60s scratch %5d B  spilled VGPRs %4d  SGPRs %5d  VGPRs %3d' % ((os.path.basename(objs[0]),) + kernels[0]))
    assert kernels[0][1] <= 128 and kernels[0][2] <= 40, kernels[0]


def test_refusals_need_no_device():
    """K or T out of range, an engine that repeats actions, host-side rules beyond one step, layer_capacity='auto' and a bad
    record are refused with rollout()'s error types before anything touches a device."""
    ok = np.zeros((2, 3, 4, 2))
    env = _engineless()
    env.observers = {}
    for K in (0, _abi.MOOG_MAX_PLAN_CANDIDATES + 1):
        with pytest.raises(ValueError, match='1 .. %d' % _abi.MOOG_MAX_PLAN_CANDIDATES):
            env.rollout_candidates(np.zeros((K, 3, 4, 2)))
    for T in (0, _abi.MOOG_MAX_ACTION_REPEAT + 1):
        with pytest.raises(ValueError, match='1 .. %d' % _abi.MOOG_MAX_ACTION_REPEAT):
            env.rollout_candidates(np.zeros((2, T, 4, 2)))
    with pytest.raises(ValueError, match=r'leading \[K, T'):
        env.rollout_candidates(np.zeros((4, 2)))
    with pytest.raises(KeyError, match='nope'):
        env.rollout_candidates(ok, record='nope')
    env._action_repeat = 2
    with pytest.raises(NotImplementedError, match='action_repeat=2'):
        env.rollout_candidates(ok)
    with pytest.raises(NotImplementedError, match='host-side meta-state rules'):
        _engineless(**_meta_config()).rollout_candidates(ok)
    auto = _engineless()
    auto._auto_capacity = True
    with pytest.raises(NotImplementedError, match="layer_capacity='auto'"):
        auto.rollout_candidates(ok)


def test_both_environments_plan():
    for cls in (environment.BatchedEnvironment, environment.SubBatchedEnvironment):
        p = inspect.signature(cls.rollout_candidates).parameters
        assert list(p) == ['self', 'actions', 'record'] and p['record'].default is None, cls
    p = inspect.signature(environment.BatchedEnvironment._rollout_candidates_packed).parameters
    assert list(p) == ['self', 'a', 'rewards', 'count', 'ended', 'traj'] and p['traj'].default is None
    assert 'bit for bit' in environment.BatchedEnvironment.rollout_candidates.__doc__
    from moog import sharding
    assert not hasattr(sharding.MultiDeviceEnvironment, 'rollout_candidates')   # (out of scope)
