"""Coverage recipe (not a reference task): a config with RaySensor observers (moog/observers/ray_sensor.py) -- egocentric
range readings from the agent.  The reference has no such observer.  Not in NAMES: the tests that iterate NAMES expect one
observer.

Walls, a `shapes` layer of mixed polygons (triangle, square, star, circle, a spoke; one of them spins, one has opacity 0 and
is seen only by a sensor with visible_only=False), a `prey` layer that a rule appends to and the agent's contact removes
from, and an agent that starts at a random angle and turns slowly, so that a sensor with follow_angle sweeps the scene.

Observers: 'image' (PILRenderer), 'table' (SpriteTable over the sensors' layers: id v of 'rays' is row v - 1 of it), 'rays'
(32 rays all round, instance ids, fixed directions) and 'front' (a 90 degree fan of 16 float16 rays that follows the
agent's angle, layer ids, opacity-0 sprites included).
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
from moog.state_initialization import distributions as distribs
from moog.state_initialization import sprite_generators

TIMEOUT_STEPS = 24
LAYER_CAPACITY = {'prey': TIMEOUT_STEPS}   # (at most one prey is created per step of an episode)
SENSOR_LAYERS = ('walls', 'shapes', 'prey', 'agent')


def sensors():
    """{key: RaySensor arguments} of the config."""
    return {
        'rays': dict(origin_layer='agent', num_rays=32, max_range=1.5, layers=SENSOR_LAYERS, mode='instance'),
        'front': dict(origin_layer='agent', num_rays=16, fov=np.pi / 2, max_range=0.75, follow_angle=True,
                      layers=SENSOR_LAYERS, mode='layer', visible_only=False, dtype='float16'),
    }


def get_config(level=0, image_size=None):
    del level
    mixed = distribs.Product(
        [distribs.Continuous('x', 0.12, 0.88), distribs.Continuous('y', 0.12, 0.88),
         distribs.Discrete('shape', ['triangle', 'square', 'star_5', 'circle', 'spoke_4']),
         distribs.Continuous('angle', 0., 2 * np.pi), distribs.Continuous('scale', 0.06, 0.16),
         distribs.Continuous('c0', 0., 1.),
         distribs.Continuous('x_vel', -0.02, 0.02), distribs.Continuous('y_vel', -0.02, 0.02)],
        c1=0.8, c2=0.9)
    make_mixed = sprite_generators.generate_sprites(mixed, num_sprites=5)
    agent_factors = distribs.Product(
        [distribs.Continuous('x', 0.3, 0.7), distribs.Continuous('y', 0.3, 0.7), distribs.Continuous('angle', 0.1, 6.1)],
        shape='triangle', scale=0.07, angle_vel=0.05, c0=0.05, c1=0.9, c2=0.9)
    make_agent = sprite_generators.generate_sprites(agent_factors, num_sprites=1)
    prey_factors = distribs.Product(
        [distribs.Continuous('x', 0.1, 0.9), distribs.Continuous('y', 0.1, 0.9), distribs.Discrete('shape', ['square', 'star_5'])],
        scale=0.08, c0=0.30, c1=0.9, c2=0.9)
    make_prey = sprite_generators.generate_sprites(prey_factors, num_sprites=1)

    def state_initializer():
        walls = shapes.border_walls(visible_thickness=0.04, c0=0.20, c1=0.9, c2=0.9)
        fixed = [sprite.Sprite(x=0.25, y=0.75, shape='hexagon', scale=0.12, angle_vel=0.3, c0=0.60, c1=0.9, c2=0.9),   # spins
                 sprite.Sprite(x=0.7, y=0.3, shape='square', scale=0.2, c0=0.80, c1=0.9, c2=0.9, opacity=0)]
        return collections.OrderedDict([('walls', walls), ('shapes', fixed + make_mixed()), ('prey', []),
                                        ('agent', make_agent())])

    rules = (
        game_rules.ConditionalRule(condition=lambda state: np.random.binomial(1, p=0.3),
                                   rules=game_rules.CreateSprites('prey', make_prey)),
        game_rules.VanishOnContact(vanishing_layer='prey', contacting_layer='agent'),
    )
    physics = physics_lib.Physics(
        (physics_lib.Drag(coeff_friction=0.25), 'agent'),
        (physics_lib.Collision(elasticity=1., symmetric=False, update_angle_vel=False), ['shapes', 'agent'], 'walls'),
        updates_per_env_step=2)
    obs = {'image': observers.PILRenderer(image_size=tuple(image_size or (64, 64)), anti_aliasing=1, color_to_rgb='hsv_to_rgb'),
           'table': observers.SpriteTable(layers=SENSOR_LAYERS, columns=('alive', 'x', 'y'))}
    for key, kw in sensors().items():
        obs[key] = observers.RaySensor(**kw)
    return {
        'state_initializer': state_initializer,
        'physics': physics,
        'task': tasks.CompositeTask(timeout_steps=TIMEOUT_STEPS),
        'action_space': action_spaces.Joystick(scaling_factor=0.02, action_layers='agent'),
        'observers': obs,
        'game_rules': rules,
    }
