"""RaySensor observer: egocentric range readings, cast on the device.

The reference hands a state-based agent the state itself (observers/raw_state.py:17-19) and leaves the featurising to the
caller.  `RaySensor` is the short egocentric vector such an agent usually wants: "how far, and to what, along each of R
directions from me" -- a `[num_envs, num_rays, 2]` float32 / float16 tensor, rewritten in place by every reset() / step() /
observation() of a `BatchedEnvironment` in one kernel launch (include/moog_engine.h moog_engine_add_sensor;
csrc/moog_ray_sensor.h states the arithmetic).

Channel 0 of a ray is the distance from the origin sprite's `position` to the nearest edge of a target polygon along the ray,
`max_range` when nothing is hit within `max_range`; channel 1 is what was hit, 0 for nothing.  mode='instance': id = 1 + row,
rows being the sprite slots of the chosen layers, layer after layer -- the numbering of `SpriteTable(layers=...)` rows, so id v
is row v - 1 of a table over the same layers (`env.ray_rows(key)` names the rows).  mode='layer': id = 1 + position of the
sprite's layer in the chosen layers.  The origin sprite is never a target; with `visible_only` a sprite of opacity 0 is none
either.  If the origin slot holds no live sprite, every ray reads (max_range, 0).

Ray k of `num_rays` points along `heading + fov * ((k + 0.5) / num_rays - 0.5)` (radians, counter-clockwise from +x; the
default heading pi/2 is a sprite's "up"); the unit vectors are computed here in float64 and handed to the engine as data
(`env.ray_directions(key)`).  With `follow_angle` the device rotates them by the origin sprite's `angle`.

Geometry not handled: no torus wrap-around and no polygon modifier.  Rays run in arena coordinates over the records' vertices:
a sprite a `TorusGeometry` renderer would draw a second time across the border is seen only where its vertices are, and a
`FirstPersonAgent` renderer's recentring does not apply.
"""
import math

import numpy as np

from .. import _abi
from .. import _dm_env as dm_env
from . import _rows

MODES = {'instance': _abi.MOOG_SENSOR_INSTANCE, 'layer': _abi.MOOG_SENSOR_LAYER}
FLOAT16_MAX = 65504.0


def sensor_dtype(sensor):
    """numpy dtype of a lowered sensor (_abi.Sensor)."""
    return _rows.numpy_dtype(sensor.dtype)


def sensor_spec(sensor, name=None):
    return dm_env.specs.Array(shape=(int(sensor.n_rays), 2), dtype=sensor_dtype(sensor), name=name)


class RaySensor(object):
    def __init__(self, origin_layer, origin_index=0, num_rays=32, fov=2 * np.pi, heading=np.pi / 2, max_range=1.0,
                 follow_angle=False, layers=None, mode='instance', visible_only=True, dtype='float32'):
        """origin_layer, origin_index: the sprite the rays start from.  num_rays: 1 .. 256.  fov: the fan's opening in
        (0, 2 pi], centred on `heading`.  max_range: finite, > 0 (at most 65504 for float16).  follow_angle: rotate the fan
        with the origin sprite.  layers: None (every layer of the state, in its order) or a tuple of layer names, used in the
        given order.  mode: 'instance' or 'layer'.  visible_only: sprites of opacity 0 are no targets.  dtype: 'float32' or
        'float16'."""
        if not isinstance(origin_layer, str):
            raise ValueError('RaySensor: origin_layer is a layer name, got %r' % (origin_layer,))
        if isinstance(origin_index, bool) or int(origin_index) != origin_index or origin_index < 0:
            raise ValueError('RaySensor: origin_index must be a non-negative integer, got %r' % (origin_index,))
        if isinstance(num_rays, bool) or int(num_rays) != num_rays or not 1 <= num_rays <= _abi.MOOG_MAX_RAYS:
            raise ValueError('RaySensor: num_rays must be an integer in 1 .. %d (MOOG_MAX_RAYS), got %r'
                             % (_abi.MOOG_MAX_RAYS, num_rays))
        fov, heading, max_range = float(fov), float(heading), float(max_range)
        if not 0.0 < fov <= 2 * math.pi:   # (a NaN fails it)
            raise ValueError('RaySensor: fov must lie in (0, 2 pi], got %r' % (fov,))
        if not math.isfinite(heading):
            raise ValueError('RaySensor: heading is not finite (%r): a direction would not be finite' % (heading,))
        if not (math.isfinite(max_range) and max_range > 0.0):
            raise ValueError('RaySensor: max_range must be finite and above 0, got %r' % (max_range,))
        if mode not in MODES:
            raise ValueError("RaySensor: unknown mode %r (modes are 'instance' and 'layer')" % (mode,))
        dtype = _rows.check_dtype('RaySensor', dtype)
        if dtype == 'float16' and max_range > FLOAT16_MAX:
            raise ValueError('RaySensor: max_range %r is above 65504: the no-hit reading would be inf as float16' % (max_range,))
        self._layers = None if layers is None else _rows.check_layers('RaySensor', layers)
        self._origin_layer, self._origin_index = origin_layer, int(origin_index)
        self._num_rays, self._fov, self._heading, self._max_range = int(num_rays), fov, heading, max_range
        self._follow_angle, self._visible_only = bool(follow_angle), bool(visible_only)
        self._mode, self._dtype = mode, dtype
        k = np.arange(self._num_rays, dtype=np.float64)
        theta = heading + fov * ((k + 0.5) / self._num_rays - 0.5)
        self._directions = np.stack([np.cos(theta), np.sin(theta)], axis=1)
        if not np.all(np.isfinite(self._directions)):
            raise ValueError('RaySensor: a direction is not finite')

    @property
    def layers(self):
        return self._layers

    @property
    def mode(self):
        return self._mode

    @property
    def num_rays(self):
        return self._num_rays

    @property
    def max_range(self):
        return self._max_range

    @property
    def dtype(self):
        return np.dtype(self._dtype)

    @property
    def directions(self):
        """[num_rays, 2] float64 unit vectors, before any rotation by the origin's angle."""
        return self._directions.copy()

    def lower(self, program, layer_names):
        """(_abi.Sensor, [(layer name, index in layer)] per row) of this observer over a lowered program: the rows are
        `SpriteTable(layers=...).lower`'s."""
        layer_names = list(layer_names)
        slots, rows = _rows.layer_rows('RaySensor', program, layer_names, self._layers)
        if self._mode == 'instance' and len(rows) > 255:
            raise NotImplementedError(
                'RaySensor: more than 255 rows in instance mode (an id is 1 .. 255, 0 is "no hit"): choose fewer '
                "layers, or mode='layer'")
        T = _abi.Sensor()
        for k, s in enumerate(slots):
            T.row_slot[k] = s
        if self._origin_layer not in layer_names:
            raise ValueError('RaySensor: unknown origin_layer %r (the state has %s)'
                             % (self._origin_layer, ', '.join(layer_names)))
        li = layer_names.index(self._origin_layer)
        if self._origin_index >= int(program.layer_nslots[li]):
            raise ValueError('RaySensor: origin_index %d is beyond the %d sprite slots of layer %r'
                             % (self._origin_index, int(program.layer_nslots[li]), self._origin_layer))
        T.origin_slot = int(program.layer_slot0[li]) + self._origin_index
        T.n_rows, T.n_rays = len(rows), self._num_rays
        T.flags = ((_abi.MOOG_SENSOR_FOLLOW_ANGLE if self._follow_angle else 0)
                   | (_abi.MOOG_SENSOR_VISIBLE_ONLY if self._visible_only else 0))
        T.mode, T.dtype, T.max_range = MODES[self._mode], _rows.DTYPES[self._dtype], self._max_range
        for k in range(self._num_rays):
            T.dirs[k][0], T.dirs[k][1] = float(self._directions[k, 0]), float(self._directions[k, 1])
        return T, rows

    def observation_spec(self):
        """specs.Array((num_rays, 2), dtype)."""
        return dm_env.specs.Array(shape=(self._num_rays, 2), dtype=np.dtype(self._dtype))
