"""Coverage recipe (not a reference task): configs with several observers -- the reference's Environment.observation()
returns {key: observer(state)} for every entry of config['observers'] (moog/environment.py:128-131), any number of
PILRenderers among them, or none.  The first PILRenderer is the engine's primary view, each further one an extra view
(include/moog_engine.h moog_engine_add_view); pinned by golden vectors captured from the reference
(tests/golden/views_zoo_l*.npz).  Not in NAMES: the tests that iterate NAMES expect one renderer per config.
level 0: colliding_predators, 'image' 64 x 64 hsv + 'ego' 48 x 48 FirstPersonAgent('agent') + 'video' 96 x 96
         anti_aliasing 2 + 'state' RawState;
level 1: chase_avoid_torus, its torus primary + a plain 64 x 64 view;
level 2: colliding_predators, a 64 x 64 primary + a 256 x 256 view (several tiles: the span kernel);
level 3: colliding_predators with a RawState observer only (no frames)."""
from moog import observers
from moog.observers import polygon_modifiers

from . import chase_avoid_torus, colliding_predators


def get_config(level):
    if level in (0, 2, 3):
        config = colliding_predators.get_config(None)
    elif level == 1:
        config = chase_avoid_torus.get_config(0)
    else:
        raise ValueError('Invalid level {}'.format(level))
    primary = config['observers']['image']
    if level == 0:
        config['observers'] = {
            'image': primary,
            'ego': observers.PILRenderer(image_size=(48, 48), anti_aliasing=1, color_to_rgb='hsv_to_rgb',
                                         polygon_modifier=polygon_modifiers.FirstPersonAgent(agent_layer='agent')),
            'video': observers.PILRenderer(image_size=(96, 96), anti_aliasing=2, color_to_rgb='hsv_to_rgb'),
            'state': observers.RawState(),
        }
    elif level == 1:
        config['observers'] = {'image': primary, 'plain': observers.PILRenderer(image_size=(64, 64), anti_aliasing=1)}
    elif level == 2:
        config['observers'] = {'image': primary,
                               'big': observers.PILRenderer(image_size=(256, 256), anti_aliasing=1, color_to_rgb='hsv_to_rgb')}
    else:
        config['observers'] = {'state': observers.RawState()}
    return config
