"""Coverage recipe (not a reference task): configs with Segmentation observers (moog/observers/segmentation.py) -- per-pixel
sprite ids of the frame.  The reference has no such observer; what it would draw is defined through its own PILRenderer
(colour = id, opacity 255, sprites of opacity 0 left out), which is how tests/golden/make_golden_segmentation.py records
the `ids_<key>` arrays of tests/golden/seg_zoo_l*.npz.  Not in NAMES: the tests that iterate NAMES expect one observer.

`segmentations(level)` says which Segmentation observers a level has ({key: arguments}); `get_config` adds them where the
`moog` package in use has the class (the reference's has not: the generator reads the arguments instead).

level 0: 64 x 64.  Walls, a `back` layer of large overlapping squares (one translucent, one of opacity 0, one shape
         partly off the canvas), movers on top, an agent.  'seg': instance ids over every layer; 'seg_layer': layer ids over
         (movers, agent) -- walls and back still occlude, and show as 0.
level 1: 40 x 24 (a width that is no multiple of 16), TorusGeometry: sprites across all four edges and a corner.
level 2: 33 x 50, FirstPersonAgent('agent').
level 3: 128 x 128, 32 sprites (two mask words, several passes over the row records), one of them a 100-vertex annulus.
level 4: 64 x 64, layers that rules append to (CreateSprites) and remove from (VanishOnContact, a timed purge), with a
         SpriteTable over the same layers: mask value v is table row v - 1.
level 5: every sprite opaque, sprite k of the state coloured (k + 1, 0, 0) under an identity colour map on black: channel 0
         of the frame IS the instance mask.  Not recorded; `image_size` chooses the size.
"""
import collections

import numpy as np

from moog import action_spaces
from moog import game_rules
from moog import observers
from moog import physics as physics_lib
from moog import shapes
from moog import sprite
from moog import tasks
from moog.observers import polygon_modifiers
from moog.state_initialization import distributions as distribs
from moog.state_initialization import sprite_generators

_SIZES = {0: (64, 64), 1: (40, 24), 2: (33, 50), 3: (128, 128), 4: (64, 64), 5: (64, 64)}


def _modifier(level):
    if level == 1:
        return polygon_modifiers.TorusGeometry(['edges', 'movers', 'agent'])
    if level == 2:
        return polygon_modifiers.FirstPersonAgent(agent_layer='agent')
    return None


def segmentations(level, image_size=None):
    """{key: Segmentation arguments} of a level (the polygon modifier is the level's renderer's: `_modifier(level)`)."""
    size = tuple(image_size or _SIZES[level])
    segs = {'seg': dict(image_size=size, layers=None, mode='instance')}
    if level == 0:
        segs['seg_layer'] = dict(image_size=size, layers=('movers', 'agent'), mode='layer')
    if level == 4:
        segs['seg'] = dict(image_size=size, layers=('prey', 'agent', 'predators'), mode='instance')
    return segs


def _movers(n, scale=(0.08, 0.18), opacity=(255,), vel=0.03):
    factors = distribs.Product(
        [distribs.Continuous('x', 0.15, 0.85), distribs.Continuous('y', 0.15, 0.85),
         distribs.Discrete('shape', ['triangle', 'star_5', 'circle', 'square', 'spoke_4']),
         distribs.Continuous('angle', 0., 2 * np.pi), distribs.Continuous('scale', *scale),
         distribs.Continuous('c0', 0., 1.),
         distribs.Discrete('opacity', list(opacity)),
         distribs.Continuous('x_vel', -vel, vel), distribs.Continuous('y_vel', -vel, vel),
         distribs.Continuous('angle_vel', -0.1, 0.1)],
        c1=0.8, c2=0.9)
    return sprite_generators.generate_sprites(factors, num_sprites=n)


def _agent():
    return sprite.Sprite(x=0.5, y=0.45, shape='square', scale=0.08, c0=0.05, c1=0.9, c2=0.9)


def _level0():
    make_movers = _movers(5, opacity=(255, 255, 150))

    def state_initializer():
        walls = shapes.border_walls(visible_thickness=0.04, c0=0.20, c1=0.9, c2=0.9)
        back = [sprite.Sprite(x=0.35, y=0.4, shape='square', scale=0.45, c0=0.40, c1=0.9, c2=0.9),
                sprite.Sprite(x=0.55, y=0.55, shape='square', scale=0.4, angle=0.5, c0=0.20, c1=0.9, c2=0.9, opacity=128),
                sprite.Sprite(x=0.6, y=0.3, shape='square', scale=0.35, c0=0.05, c1=0.9, c2=0.9, opacity=0),
                sprite.Sprite(x=0.97, y=0.7, shape='star_5', scale=0.3, c0=0.50, c1=0.9, c2=0.9)]
        return collections.OrderedDict([('walls', walls), ('back', back), ('movers', make_movers()), ('agent', [_agent()])])

    physics = physics_lib.Physics(
        (physics_lib.Drag(coeff_friction=0.1), 'agent'),
        (physics_lib.Collision(elasticity=1., symmetric=False, update_angle_vel=True), ['movers', 'agent'], 'walls'),
        updates_per_env_step=3)
    return state_initializer, (), physics, tasks.CompositeTask(timeout_steps=14)


def _level1():
    make_movers = _movers(6, scale=(0.1, 0.25), opacity=(255, 255, 120), vel=0.05)

    def state_initializer():
        # across the left, right, bottom and top edges, and across a corner: the torus copies show on the other side
        edges = [sprite.Sprite(x=0.0, y=0.5, shape='square', scale=0.2, x_vel=0.01, c0=0.70, c1=0.9, c2=0.9),
                 sprite.Sprite(x=1.0, y=0.25, shape='triangle', scale=0.2, y_vel=0.01, c0=0.90, c1=0.9, c2=0.9),
                 sprite.Sprite(x=0.35, y=0.0, shape='circle', scale=0.12, x_vel=-0.01, c0=0.50, c1=0.9, c2=0.9),
                 sprite.Sprite(x=0.7, y=1.0, shape='star_5', scale=0.2, y_vel=-0.01, c0=0.80, c1=0.9, c2=0.9, opacity=180),
                 sprite.Sprite(x=0.02, y=0.97, shape='square', scale=0.22, angle=0.3, x_vel=-0.005, y_vel=0.005,
                               c0=0.40, c1=0.9, c2=0.9)]
        return collections.OrderedDict([('edges', edges), ('movers', make_movers()), ('agent', [_agent()])])

    physics = physics_lib.Physics((physics_lib.Drag(coeff_friction=0.1), 'agent'), updates_per_env_step=2)
    return state_initializer, (), physics, tasks.CompositeTask(timeout_steps=14)


def _level2():
    make_movers = _movers(5, opacity=(255, 200))

    def state_initializer():
        back = [sprite.Sprite(x=0.3, y=0.3, shape='square', scale=0.4, c0=0.40, c1=0.9, c2=0.9),
                sprite.Sprite(x=0.75, y=0.7, shape='hexagon', scale=0.25, c0=0.20, c1=0.9, c2=0.9, opacity=128),
                sprite.Sprite(x=0.2, y=0.85, shape='triangle', scale=0.3, c0=0.50, c1=0.9, c2=0.9)]
        return collections.OrderedDict([('back', back), ('movers', make_movers()), ('agent', [_agent()])])

    physics = physics_lib.Physics((physics_lib.Drag(coeff_friction=0.05), 'agent'), updates_per_env_step=2)
    return state_initializer, (), physics, tasks.CompositeTask(timeout_steps=14)


def _level3():
    make_movers = _movers(26, scale=(0.06, 0.16), opacity=(255, 255, 255, 140))

    def state_initializer():
        walls = shapes.border_walls(visible_thickness=0.03, c0=0.20, c1=0.9, c2=0.9)
        ring = sprite.Sprite(x=0.5, y=0.5, shape=shapes.annulus_vertices(inner_radius=0.2, outer_radius=0.3), scale=1.,
                             c0=0.60, c1=0.9, c2=0.9, opacity=200)
        return collections.OrderedDict([('walls', walls), ('movers', make_movers()), ('agent', [_agent()]),
                                        ('ring', [ring])])

    physics = physics_lib.Physics(
        (physics_lib.Drag(coeff_friction=0.1), ['agent', 'ring']),
        (physics_lib.Collision(elasticity=1., symmetric=False, update_angle_vel=True), ['movers', 'agent'], 'walls'),
        updates_per_env_step=2)
    return state_initializer, (), physics, tasks.CompositeTask(timeout_steps=16)


def _level4():
    rng = [-0.05, 1.05]
    boundary = distribs.Mixture([
        distribs.Product([distribs.Continuous('y', *rng)], x=rng[0]),
        distribs.Product([distribs.Continuous('y', *rng)], x=rng[1]),
        distribs.Product([distribs.Continuous('x', *rng)], y=rng[0]),
        distribs.Product([distribs.Continuous('x', *rng)], y=rng[1]),
    ])
    predator_factors = distribs.Product(
        [boundary, distribs.Continuous('x_vel', -0.03, 0.03), distribs.Continuous('y_vel', -0.03, 0.03),
         distribs.Continuous('scale', 0.1, 0.2)],
        shape='circle', c0=0.90, c1=0.9, c2=0.9)
    prey_factors = distribs.Product(
        [distribs.Continuous('x', 0.1, 0.9), distribs.Continuous('y', 0.1, 0.9),
         distribs.Discrete('shape', ['square', 'star_5'])],
        scale=0.12, c0=0.20, c1=0.9, c2=0.9)
    predator_gen = sprite_generators.generate_sprites(predator_factors, num_sprites=1)
    prey_gen = sprite_generators.generate_sprites(prey_factors, num_sprites=1)

    def state_initializer():
        walls = shapes.border_walls(visible_thickness=0.03, c0=0.20, c1=0.9, c2=0.9)
        agent = sprite.Sprite(x=0.5, y=0.5, shape='circle', scale=0.1, c0=0.05, c1=0.9, c2=0.9)
        return collections.OrderedDict([('walls', walls), ('prey', []), ('agent', [agent]), ('predators', [])])

    rules = (
        game_rules.ConditionalRule(condition=lambda state: np.random.binomial(1, p=0.5),
                                   rules=game_rules.CreateSprites('predators', predator_gen)),
        game_rules.ConditionalRule(condition=lambda state: np.random.binomial(1, p=0.3),
                                   rules=game_rules.CreateSprites('prey', prey_gen)),
        game_rules.VanishOnContact(vanishing_layer='prey', contacting_layer='agent'),
        game_rules.TimedRule((6, 8), (game_rules.VanishByFilter('predators'),)),
    )
    physics = physics_lib.Physics(
        (physics_lib.Drag(coeff_friction=0.25), 'agent'),
        (physics_lib.Collision(elasticity=0.5, symmetric=False), 'agent', 'walls'),
        updates_per_env_step=3)
    return state_initializer, rules, physics, tasks.CompositeTask(timeout_steps=12)


def _level5():
    n_movers = 12

    def mover(k):
        factors = distribs.Product(
            [distribs.Continuous('x', 0.15, 0.85), distribs.Continuous('y', 0.15, 0.85),
             distribs.Discrete('shape', ['triangle', 'star_5', 'circle', 'square']),
             distribs.Continuous('angle', 0., 2 * np.pi), distribs.Continuous('scale', 0.1, 0.25),
             distribs.Continuous('x_vel', -0.04, 0.04), distribs.Continuous('y_vel', -0.04, 0.04)],
            c0=k + 1, c1=0, c2=0)
        return sprite_generators.generate_sprites(factors, num_sprites=1)

    makers = [mover(4 + k) for k in range(n_movers)]

    def state_initializer():
        walls = [shapes.border_walls(visible_thickness=0.04, c0=k + 1, c1=0, c2=0)[k] for k in range(4)]
        movers = []
        for make in makers:
            movers.extend(make())
        agent = sprite.Sprite(x=0.5, y=0.45, shape='square', scale=0.1, c0=4 + n_movers + 1, c1=0, c2=0)
        return collections.OrderedDict([('walls', walls), ('movers', movers), ('agent', [agent])])

    physics = physics_lib.Physics(
        (physics_lib.Drag(coeff_friction=0.1), 'agent'),
        (physics_lib.Collision(elasticity=1., symmetric=True, update_angle_vel=True), 'movers', 'movers'),
        (physics_lib.Collision(elasticity=1., symmetric=False, update_angle_vel=True), ['movers', 'agent'], 'walls'),
        updates_per_env_step=3)
    return state_initializer, (), physics, tasks.CompositeTask(timeout_steps=9)


def get_config(level, image_size=None):
    if level not in _SIZES:
        raise ValueError('Invalid level {}'.format(level))
    state_initializer, rules, physics, task = (_level0, _level1, _level2, _level3, _level4, _level5)[level]()
    size = tuple(image_size or _SIZES[level])
    layers = ('agent', 'ring') if level == 3 else 'agent'
    obs = {'image': observers.PILRenderer(image_size=size, anti_aliasing=1, color_to_rgb=None if level == 5 else 'hsv_to_rgb',
                                          polygon_modifier=_modifier(level))}
    if hasattr(observers, 'Segmentation'):
        for key, kw in segmentations(level, size).items():
            obs[key] = observers.Segmentation(polygon_modifier=_modifier(level), **kw)
    if level == 4 and hasattr(observers, 'SpriteTable'):
        obs['table'] = observers.SpriteTable(layers=('prey', 'agent', 'predators'), columns=('alive', 'x', 'y'))
    return {
        'state_initializer': state_initializer,
        'physics': physics,
        'task': task,
        'action_space': action_spaces.Joystick(scaling_factor=0.02, action_layers=layers),
        'observers': obs,
        'game_rules': rules,
    }
