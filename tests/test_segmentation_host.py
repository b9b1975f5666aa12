"""Segmentation observer without a GPU: how a config with one lowers (rows, ids per sprite slot, modifier), what is refused
and why, the observation spec, and that the program -- bytes and hash -- does not know about it.  The device code's host
model is tests/test_segmentation_model.py, the kernel itself tests/test_segmentation_gpu.py."""
import ctypes

import numpy as np
import pytest

import helpers
from moog import _abi, _compiler, _engine, observers
from moog.observers import polygon_modifiers
from moog_demos import example_configs
from moog_demos.example_configs import seg_zoo


def compile_with(name, extra, capacity=None):
    cfg = example_configs.load(name)
    cfg['observers'] = dict(cfg['observers'], **extra)
    return _compiler.compile_config(layer_capacity=capacity or example_configs.capacity(name), **cfg)


def program_hash(c):
    lib = _engine.load_library()
    h = ctypes.c_uint64()
    _engine.check(lib, lib.moog_program_step_kernel(ctypes.byref(c.program), None, None, ctypes.byref(h)))
    return h.value


def slot_ids(G, n):
    return [int(G.slot_id[s]) for s in range(n)]


@pytest.mark.parametrize('name,layers', [('colliding_predators_32', None), ('colliding_predators_32', ('predators', 'agent')),
                                         ('rules_zoo_l1', ('prey', 'predators')), ('pong', None)])
def test_rows_are_the_sprite_tables(name, layers):
    """Rows = the slots of the chosen layers, layer after layer: SpriteTable(layers=...)'s; instance ids = 1 + row at the
    row's slot and 0 at every other slot; layer ids = 1 + the layer's position among the chosen ones."""
    c = compile_with(name, {'seg': observers.Segmentation(layers=layers), 'lay': observers.Segmentation(layers=layers, mode='layer'),
                            'table': observers.SpriteTable(layers=layers)})
    P = c.program
    T = dict(c.tables)['table']
    segs = dict(c.segmentations)
    assert list(segs) == ['seg', 'lay']
    assert c.segmentation_rows['seg'] == c.table_rows['table'] == c.segmentation_rows['lay']
    want = [0] * P.n_slots
    for r in range(T.n_rows):
        want[T.row_slot[r]] = 1 + r
    assert slot_ids(segs['seg'], P.n_slots) == want
    chosen = list(c.layer_names) if layers is None else list(layers)
    want = [1 + chosen.index(c.layer_names[P.slot_layer[s]]) if c.layer_names[P.slot_layer[s]] in chosen else 0
            for s in range(P.n_slots)]
    assert slot_ids(segs['lay'], P.n_slots) == want
    for G in segs.values():
        assert (G.width, G.height, G.polymod, G.n_slots) == (64, 64, _abi.MOOG_POLYMOD_NONE, P.n_slots)
        assert not any(G.slot_id[s] for s in range(P.n_slots, _abi.MOOG_MAX_SLOTS))


def test_modifiers_and_sizes_lower_like_a_renderers():
    c = compile_with('colliding_predators', {
        'torus': observers.Segmentation(image_size=(40, 24), polygon_modifier=polygon_modifiers.TorusGeometry(['agent'])),
        'ego': observers.Segmentation(image_size=(33, 50), polygon_modifier=polygon_modifiers.FirstPersonAgent(agent_layer='agent'))})
    torus, ego = dict(c.segmentations)['torus'], dict(c.segmentations)['ego']
    assert (torus.width, torus.height, torus.polymod) == (40, 24, _abi.MOOG_POLYMOD_TORUS)
    assert (ego.width, ego.height, ego.polymod, ego.polymod_layer) == (33, 50, _abi.MOOG_POLYMOD_FIRST_PERSON, c.layer_names.index('agent'))
    for level in (0, 1, 2, 3, 4):   # the recipe's levels lower, with the renderer's own modifier
        cl = _compiler.compile_config(**seg_zoo.get_config(level))
        R = cl.program.render
        for key, G in cl.segmentations:
            assert (G.width, G.height, G.polymod, G.polymod_layer) == (R.width, R.height, R.polymod, R.polymod_layer), (level, key)


def test_observation_spec():
    seg = observers.Segmentation(image_size=(40, 24))
    spec = seg.observation_spec()
    assert spec.shape == (24, 40) and spec.dtype == np.uint8
    assert observers.Segmentation().observation_spec().shape == (64, 64)
    cfg = seg_zoo.get_config(1)
    assert {k: (o.observation_spec().shape, o.observation_spec().dtype) for k, o in cfg['observers'].items()} == {
        'image': ((40, 24, 3), np.uint8), 'seg': ((24, 40), np.uint8)}


@pytest.mark.parametrize('name', ('pong', 'colliding_predators_32', 'rules_zoo_l1', 'chase_avoid_torus'))
def test_program_does_not_know(name):
    """Bytes and hash of the program (what the specialised step kernels are keyed by) with and without the observer."""
    plain = helpers.compiled(name)
    c = compile_with(name, {'seg': observers.Segmentation(), 'lay': observers.Segmentation(image_size=(128, 96), mode='layer')})
    assert len(c.segmentations) == 2 and not plain.segmentations and plain.segmentation_rows == {}
    assert bytes(c.program) == bytes(plain.program) and program_hash(c) == program_hash(plain)
    assert bytes(c.layout) == bytes(plain.layout)


def test_refusals():
    """Each with a message that says why."""
    with pytest.raises(NotImplementedError, match='span rasteriser'):
        observers.Segmentation(image_size=(129, 64))
    with pytest.raises(NotImplementedError, match='span rasteriser'):
        observers.Segmentation(image_size=(64, 256))
    observers.Segmentation(image_size=(128, 128))
    with pytest.raises(ValueError, match='unknown mode'):
        observers.Segmentation(mode='semantic')
    with pytest.raises(ValueError, match='named twice'):
        observers.Segmentation(layers=('agent', 'agent'))
    with pytest.raises(ValueError, match='not one string'):
        observers.Segmentation(layers='agent')
    with pytest.raises(ValueError, match="unknown layer 'nowhere'"):
        compile_with('pong', {'seg': observers.Segmentation(layers=('nowhere',))})
    # more than MOOG_MAX_SEGMENTATIONS
    assert _abi.MOOG_MAX_SEGMENTATIONS == 2
    two = {'s%d' % k: observers.Segmentation() for k in range(2)}
    assert len(compile_with('pong', two).segmentations) == 2
    with pytest.raises(NotImplementedError, match='MOOG_MAX_SEGMENTATIONS'):
        compile_with('pong', dict(two, third=observers.Segmentation()))
    # a config without any PILRenderer: no raster state
    cfg = example_configs.load('pong')
    cfg['observers'] = {'seg': observers.Segmentation(), 'state': observers.RawState()}
    with pytest.raises(NotImplementedError, match='no PILRenderer'):
        _compiler.compile_config(**cfg)


def test_refusals_that_follow_from_the_program():
    """More than 255 rows in instance mode; a frame the mask rasteriser cannot hold (moog_engine_raster_path's criteria)."""
    c = helpers.compiled('colliding_predators_32')   # 32 slots: 288 torus copies > 256 items
    assert c.program.n_slots * 9 > 256
    with pytest.raises(NotImplementedError, match='at most 256'):
        compile_with('colliding_predators_32', {'seg': observers.Segmentation(polygon_modifier=polygon_modifiers.TorusGeometry(['agent']))})
    assert len(compile_with('colliding_predators_32', {'seg': observers.Segmentation()}).segmentations) == 1
    # the same rule as the engine's for a view: a program whose frames take the span kernel at this size has no segmentation
    G = _abi.Segmentation()
    G.width, G.height, G.n_slots = 128, 128, 256
    big = helpers.compiled('falling_balls_64')
    why = _compiler.segmentation_refusal(big.program, big.layout, G)
    lds = min(_compiler.mask_plan_bytes(big.program.n_slots, big.layout.TOTV, 128, 128, 128, False, k) for k in (False, True))
    assert (why is None) == (lds <= 64 * 1024)
    assert 'LDS' in _compiler.segmentation_refusal(big.program, _Fake(big.layout, 40000), G)
    # 255 rows at most in instance mode; layer mode has no such limit
    P = _abi.Program()
    P.n_slots, P.n_layers = 256, 1
    P.layer_slot0[0], P.layer_nslots[0] = 0, 256
    with pytest.raises(NotImplementedError, match='more than 255 rows'):
        observers.Segmentation().lower(P, ['all'])
    G, rows = observers.Segmentation(mode='layer').lower(P, ['all'])
    assert len(rows) == 256 and slot_ids(G, 256) == [1] * 256
    P.layer_nslots[0] = P.n_slots = 255
    G, rows = observers.Segmentation().lower(P, ['all'])
    assert slot_ids(G, 255) == list(range(1, 256))


class _Fake(object):
    """A layout with another vertex count (tables beyond 64 KB of LDS)."""

    def __init__(self, layout, totv):
        self.TOTV = totv


def test_symbols_and_versions():
    lib = _engine.load_library()
    for sym in ('moog_engine_add_segmentation', 'moog_engine_set_segmentation_image'):
        assert sym in _engine.SYMBOLS and hasattr(lib, sym), sym
    assert lib.moog_abi_version() == 31 == _abi.MOOG_ABI_VERSION and _abi.MOOG_PROGRAM_VERSION == 30
    assert (_abi.MOOG_K_VIEWS, _abi.MOOG_K_TABLES, _abi.MOOG_K_COUNT) == (3, 4, 5)
    assert ctypes.sizeof(_abi.Segmentation) == 5 * 4 + _abi.MOOG_MAX_SLOTS
