"""Configs with several observers (the reference's Environment.observation(), moog/environment.py:128-131, returns
{key: observer(state)} for every observer): lowering of every PILRenderer -- the first into the program, the others into
the engine's extra views -- its limits, configs without a renderer, and the multi-view recordings of the reference
(tests/golden/views_zoo_l*.npz) replayed on the oracle, one renderer at a time.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import helpers
from helpers import OracleEnv, fixture, records_from_fixture, uniforms_of
from moog import _abi, _compiler, observers
from moog.observers import polygon_modifiers
from moog_demos.example_configs import views_zoo


def _compile(cfg):
    return _compiler.compile_config(**cfg)


def _only(cfg, key):
    """The config with one observer: `key`'s renderer alone."""
    out = dict(cfg)
    out['observers'] = {key: cfg['observers'][key]}
    return out


def _fields(R):
    return (R.width, R.height, R.cmap, R.polymod, tuple(R.bg), R.polymod_layer, R.aa)


def test_extra_views_leave_the_program_alone():
    cfg = views_zoo.get_config(0)
    c = _compile(cfg)
    first = _compile(_only(cfg, 'image'))
    assert bytes(c.program) == bytes(first.program)
    assert c.observer_key == 'image'
    assert [k for k, _ in c.views] == ['ego', 'video']
    agent = c.layer_names.index('agent')
    ego, video = c.views[0][1], c.views[1][1]
    assert _fields(ego) == (48, 48, _abi.MOOG_CMAP_HSV, _abi.MOOG_POLYMOD_FIRST_PERSON, (0, 0, 0), agent, 1)
    assert _fields(video) == (96, 96, _abi.MOOG_CMAP_HSV, _abi.MOOG_POLYMOD_NONE, (0, 0, 0), 0, 2)
    # each extra view lowers to what the program's render would be with that renderer alone
    for key, R in c.views:
        assert _fields(R) == _fields(_compile(_only(cfg, key)).program.render), key


def test_torus_primary_and_plain_view():
    c = _compile(views_zoo.get_config(1))
    assert c.program.render.polymod == _abi.MOOG_POLYMOD_TORUS
    assert [k for k, _ in c.views] == ['plain']
    assert c.views[0][1].polymod == _abi.MOOG_POLYMOD_NONE and c.views[0][1].cmap == _abi.MOOG_CMAP_IDENTITY


def test_too_many_renderers_refused():
    cfg = views_zoo.get_config(0)
    cfg['observers'] = {'v%d' % k: observers.PILRenderer(image_size=(32, 32)) for k in range(_abi.MOOG_MAX_VIEWS + 1)}
    with pytest.raises(NotImplementedError, match='MOOG_MAX_VIEWS'):
        _compile(cfg)
    cfg['observers'] = {'v%d' % k: observers.PILRenderer(image_size=(32, 32)) for k in range(_abi.MOOG_MAX_VIEWS)}
    assert len(_compile(cfg).views) == _abi.MOOG_MAX_VIEWS - 1


def test_distinct_callable_colour_map_on_an_extra_view_refused():
    cfg = views_zoo.get_config(0)

    def grey(c):
        return (128, 128, 128)

    def red(c):
        return (255, 0, 0)
    cfg['observers'] = {'image': observers.PILRenderer(image_size=(32, 32), color_to_rgb=grey),
                        'other': observers.PILRenderer(image_size=(32, 32), color_to_rgb=red)}
    with pytest.raises(NotImplementedError, match='color_to_rgb'):
        _compile(cfg)
    cfg['observers']['other'] = observers.PILRenderer(image_size=(48, 48), color_to_rgb=grey)   # the same object: shared
    c = _compile(cfg)
    assert c.color_fn is grey and [k for k, _ in c.views] == ['other']


@pytest.mark.parametrize('obs', [{'state': observers.RawState()}, {}])
def test_no_renderer_draws_no_frames(obs):
    cfg = views_zoo.get_config(0)
    cfg['observers'] = obs
    c = _compile(cfg)
    assert (c.program.render.width, c.program.render.height) == (0, 0)
    assert c.observer_key is None and c.views == []
    # everything but the renderer is the same program
    with_renderer = _compile(_only(views_zoo.get_config(0), 'image'))
    a, b = _abi.Program.from_buffer_copy(bytes(c.program)), _abi.Program.from_buffer_copy(bytes(with_renderer.program))
    a.render = _abi.Render()
    b.render = _abi.Render()
    assert bytes(a) == bytes(b)
    assert views_zoo.get_config(3)['observers'].keys() == {'state'}


def test_other_observer_types_still_refused():
    cfg = views_zoo.get_config(0)
    cfg['observers'] = {'image': cfg['observers']['image'], 'odd': object()}
    with pytest.raises(NotImplementedError):
        _compile(cfg)


VIEW_KEYS = {0: ('image', 'ego', 'video'), 1: ('image', 'plain'), 2: ('image', 'big')}


@pytest.mark.parametrize('level', [0, 1, 2])
def test_oracle_views_match_reference(level):
    """Every recorded call teacher-forced on the oracle; each view drawn by the config compiled with that renderer alone
    (the layout does not depend on the renderer) equals the reference's frame bit for bit."""
    name = 'views_zoo_l%d' % level
    fx = fixture(name)
    cfg = views_zoo.get_config(level)
    base = _compile(cfg)
    T = len(fx['step_type'])
    for key in VIEW_KEYS[level]:
        c = _compile(_only(cfg, key))
        assert bytes(c.layout) == bytes(base.layout)
        o = OracleEnv(c)
        frames = fx['image_' + key]
        assert frames.shape[0] == T
        o.reset(uniforms=uniforms_of(fx, 0))
        assert np.array_equal(o.image[0], frames[0]), (key, 0)
        for t in range(1, T):
            records_from_fixture(fx, t - 1, c, o.f64, o.i32)
            o.step(helpers.action_of(fx, t), uniforms=uniforms_of(fx, t))
            assert int(o.step_type[0]) == int(fx['step_type'][t]), (key, t)
            assert np.array_equal(o.image[0], frames[t]), '%s: frame %d differs' % (key, t)
    assert np.array_equal(fx['image_image'], fx['image'])


@pytest.mark.parametrize('other', [dict(color_to_rgb='hsv_to_rgb'), dict(color_to_rgb=None)])
def test_callable_primary_with_a_plain_extra_view_refused(other):
    """The colour override holds the primary's callable colours and applies to every view: an extra view with the hsv or the
    identity map next to a callable primary would be drawn in the callable's colours, so it is refused."""
    cfg = views_zoo.get_config(0)

    def grey(c):
        return (128, 128, 128)
    cfg['observers'] = {'image': observers.PILRenderer(image_size=(32, 32), color_to_rgb=grey),
                        'big': observers.PILRenderer(image_size=(64, 64), **other)}
    with pytest.raises(NotImplementedError, match='color_to_rgb'):
        _compile(cfg)
