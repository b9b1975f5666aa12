"""SpriteTable observer: the state as one dense tensor of per-sprite features, written on the device.

The reference hands a state-based agent the state itself (observers/raw_state.py:17-19) and leaves the featurising to the
caller.  Here the state lives in the device records, and `SpriteTable` is the observer that turns them into what a network
takes: a `[num_envs, rows, columns]` float32 / float16 tensor, rewritten in place by every reset() / step() / observation()
of a `BatchedEnvironment` in one kernel launch (include/moog_engine.h moog_engine_add_table; csrc/moog_sprite_table.h).

Rows are the sprite slots of the chosen layers, layer after layer, `layer_capacity` slots for a layer that rules append to:
the row count is fixed, `env.table_rows(key)` names every row.  A live row holds the sprite's attributes as the reference
holds them (sprite.py:237-253: no normalisation, no colour map), converted with one round-to-nearest-even as
`numpy.ndarray.astype` does; the row of a slot without a live sprite is all zeros, `alive` included.  In a layer that rules
append to, live sprites are packed at the front in list order, so row i of the layer is the reference's `state[layer][i]`.
"""
import numpy as np

from .. import _abi
from .. import _dm_env as dm_env
from . import _rows

# column name -> MOOG_TCOL_* (include/moog_engine.h): the numeric Sprite.FACTOR_NAMES, then what the records hold besides
COLUMN_IDS = {
    'x': _abi.MOOG_TCOL_X, 'y': _abi.MOOG_TCOL_Y, 'angle': _abi.MOOG_TCOL_ANGLE, 'scale': _abi.MOOG_TCOL_SCALE,
    'c0': _abi.MOOG_TCOL_C0, 'c1': _abi.MOOG_TCOL_C1, 'c2': _abi.MOOG_TCOL_C2, 'opacity': _abi.MOOG_TCOL_OPACITY,
    'x_vel': _abi.MOOG_TCOL_X_VEL, 'y_vel': _abi.MOOG_TCOL_Y_VEL, 'angle_vel': _abi.MOOG_TCOL_ANGLE_VEL,
    'mass': _abi.MOOG_TCOL_MASS, 'aspect_ratio': _abi.MOOG_TCOL_ASPECT,
    'alive': _abi.MOOG_TCOL_ALIVE, 'layer': _abi.MOOG_TCOL_LAYER, 'shape_id': _abi.MOOG_TCOL_SHAPE_ID,
    'n_vertices': _abi.MOOG_TCOL_N_VERTICES,
}
NEEDS_SPRITE_FACTORS = ('scale', 'aspect_ratio')


def table_dtype(table):
    """numpy dtype of a lowered table (_abi.Table)."""
    return _rows.numpy_dtype(table.dtype)


def table_spec(table, name=None):
    return dm_env.specs.Array(shape=(int(table.n_rows), int(table.n_cols)), dtype=table_dtype(table), name=name)


class SpriteTable(object):
    ALL_COLUMNS = ('alive', 'x', 'y', 'angle', 'scale', 'c0', 'c1', 'c2', 'opacity', 'x_vel', 'y_vel', 'angle_vel', 'mass',
                   'aspect_ratio', 'layer', 'shape_id', 'n_vertices')
    DEFAULT_COLUMNS = ('alive', 'x', 'y', 'x_vel', 'y_vel', 'angle', 'angle_vel', 'c0', 'c1', 'c2', 'opacity', 'mass')

    def __init__(self, layers=None, columns=DEFAULT_COLUMNS, dtype='float32'):
        """layers: None (every layer of the state, in its order) or a tuple of layer names, used in the given order.
        columns: a tuple of names from ALL_COLUMNS (`shape`, a string, and `metadata` are not columns; `shape_id` indexes
        `compiled.shape_names`); `scale` / `aspect_ratio` need an environment built with keep_sprite_factors=True.
        dtype: 'float32' or 'float16'."""
        if isinstance(columns, str):
            raise ValueError('SpriteTable: columns is a tuple of names, not one string')
        self._layers = None if layers is None else _rows.check_layers('SpriteTable', layers)
        self._columns = tuple(columns)
        if not self._columns:
            raise ValueError('SpriteTable: no columns')
        for c in self._columns:
            if c not in COLUMN_IDS:
                raise ValueError('SpriteTable: unknown column %r (columns are %s; `shape` and `metadata` are not numeric)'
                                 % (c, ', '.join(self.ALL_COLUMNS)))
        if len(set(self._columns)) != len(self._columns):
            raise ValueError('SpriteTable: a column is named twice in %r' % (self._columns,))
        self._dtype = _rows.check_dtype('SpriteTable', dtype)
        self._table = None   # the last lowering of this observer (compile_config), for observation_spec()

    @property
    def columns(self):
        return self._columns

    @property
    def layers(self):
        return self._layers

    @property
    def dtype(self):
        return np.dtype(self._dtype)

    def lower(self, program, layer_names):
        """(_abi.Table, [(layer name, index in layer)] per row) of this observer over a lowered program."""
        if program.sprite_factors == 0:
            need = [c for c in self._columns if c in NEEDS_SPRITE_FACTORS]
            if need:
                raise ValueError('SpriteTable column%s %s: the state records hold scale / aspect_ratio only when the '
                                 'environment is built with keep_sprite_factors=True'
                                 % ('s' if len(need) > 1 else '', ', '.join(need)))
        slots, rows = _rows.layer_rows('SpriteTable', program, layer_names, self._layers)
        T = _abi.Table()
        for k, s in enumerate(slots):
            T.row_slot[k] = s
        T.n_rows, T.n_cols, T.dtype = len(rows), len(self._columns), _rows.DTYPES[self._dtype]
        for k, c in enumerate(self._columns):
            T.cols[k] = COLUMN_IDS[c]
        self._table = T
        return T, rows

    def observation_spec(self):
        """specs.Array(shape=(rows, columns), dtype): known once a config holding this observer has been lowered (an
        environment built from it, or _compiler.compile_config); `env.observation_spec()` always knows."""
        if self._table is None:
            raise ValueError('SpriteTable.observation_spec(): the row count follows from the state_initializer and '
                             'layer_capacity -- build the environment first (env.observation_spec())')
        return table_spec(self._table)
