"""Open-loop rollouts, what needs no device: the entry point moog_engine_step_sequence in the header, the binding and the
built library; the version numbers and program bytes it leaves alone; the refusals BatchedEnvironment.rollout gives before it
touches an engine."""
import ctypes
import re

import numpy as np
import pytest

import helpers
from moog import _abi, _engine, environment
from test_action_repeat import _meta_config


def test_abi_declares_the_sequence_call_and_leaves_the_programs_alone():
    assert 'moog_engine_step_sequence' in _engine.SYMBOLS
    hdr = open(_abi.HEADER).read()
    assert 'moog_engine_step_sequence' in set(re.findall(r'\b(moog_\w+)\s*\(', hdr))
    lib = _engine.load_library()
    assert hasattr(lib, 'moog_engine_step_sequence')
    # (a null engine is refused, not dereferenced -- whatever else the call is handed)
    buf = (ctypes.c_double * 8)()
    assert lib.moog_engine_step_sequence(None, ctypes.addressof(buf), 2, 16, ctypes.addressof(buf), 4, None, None, None) != 0
    assert b'null engine' in lib.moog_last_error()
    assert lib.moog_engine_step_sequence(None, None, 0, 0, None, 0, None, None, None) != 0
    assert _abi.MOOG_ABI_VERSION == 31 and _abi.MOOG_PROGRAM_VERSION == 30 and _abi.MOOG_K_COUNT == 5
    assert lib.moog_abi_version() == 31
    P = helpers.compiled('colliding_predators_32').program
    assert P.abi_version == _abi.MOOG_PROGRAM_VERSION
    h = ctypes.c_uint64()
    _engine.check(lib, lib.moog_program_step_kernel(ctypes.byref(P), None, None, ctypes.byref(h)))
    assert '%016x' % h.value == '417c47560f31861d'   # (the headline's specialised kernel keeps its name)


def _engineless(action_repeat=1, **config):
    """A BatchedEnvironment as __init__ leaves it just before it touches a device: what rollout()'s refusals read."""
    env = environment.BatchedEnvironment.__new__(environment.BatchedEnvironment)
    cap = config.get('layer_capacity')
    env._auto_capacity = cap == 'auto' or (isinstance(cap, dict) and bool(cap.get('auto')))
    env._host_rules = [r for r in config.get('game_rules', ()) if getattr(r, 'host_side', False)]
    env._meta_state_initializer = config.get('meta_state_initializer')
    env._action_repeat = action_repeat
    env._handle = None   # (nothing to destroy)
    return env


def test_rollout_refusals_need_no_device():
    """What an action repeat of T cannot do, a rollout of T actions cannot either (the same function says so), and it says so
    before anything touches a device: host-side meta-state rules, a meta_state_initializer, layer_capacity='auto'; T outside
    1 .. MOOG_MAX_ACTION_REPEAT; an engine that already repeats actions."""
    from moog_demos import example_configs
    seq = np.zeros((3, 4, 2))
    with pytest.raises(NotImplementedError, match='host-side meta-state rules'):
        _engineless(**_meta_config()).rollout(seq)
    cfg = example_configs.load('pong')
    cfg['meta_state_initializer'] = lambda: {'n': 0}
    with pytest.raises(NotImplementedError, match='meta_state_initializer'):
        _engineless(**cfg).rollout(seq)
    for cap in ('auto', {'auto': True, 'prey': 16}):
        with pytest.raises(NotImplementedError, match="layer_capacity='auto'"):
            _engineless(layer_capacity=cap, **example_configs.load('rules_zoo')).rollout(seq)
    plain = _engineless(**example_configs.load('pong'))
    for T in (0, _abi.MOOG_MAX_ACTION_REPEAT + 1):
        with pytest.raises(ValueError, match='1 .. %d' % _abi.MOOG_MAX_ACTION_REPEAT):
            plain.rollout(np.zeros((T, 4, 2)))
    with pytest.raises(ValueError):
        plain.rollout({})
    with pytest.raises(NotImplementedError, match='action_repeat=2'):
        _engineless(action_repeat=2, **example_configs.load('pong')).rollout(seq)
    assert hasattr(environment.SubBatchedEnvironment, 'rollout')
