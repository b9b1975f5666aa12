"""Contacts observer: per-pair overlap flags, computed on the device.

Contact is what the tasks are made of: `ContactReward`, `contact_rules`, the `Vanish*` rules and the config-local rules of
`cleanup` and `functional_maze` all ask `sprite.overlaps_sprite(other)`, and the engine evaluates that predicate inside its
step kernel without ever showing an answer.  `Contacts` shows it: who is touching whom, as a uint8 device tensor in every
timestep, rewritten in place by every reset() / step() / observation() of a `BatchedEnvironment` in one kernel launch
(include/moog_engine.h moog_engine_add_contacts; csrc/moog_contacts.h states the predicate and the kernel).

`Contacts(layers_0, layers_1=None, mode='pair' | 'layer', visible_only=False)`

layers_0, layers_1: a layer name or a tuple of names, each known to the state and not repeated within one argument.
    `layers_1=None` means `layers_0`.  Rows are the layers' sprite slots, layer after layer, exactly as a
    `SpriteTable(layers=...)` over the same layers numbers them; `env.contact_rows(key)` returns `(rows_0, rows_1)` as
    lists of `(layer, index)`.  R0 and R1 are the two row counts.

mode='pair': `[num_envs, R0, R1]` uint8.  Entry `[e, i, j]` is 1 iff in env `e`
    * row i's slot and row j's slot are both alive,
    * they are different slots,
    * with `visible_only`, both have opacity > 0, and
    * `state[row i].overlaps_sprite(state[row j])` holds on the record as it stands;
    otherwise it is 0.

mode='layer': `[num_envs, R0, n_layers_1]` uint8.  Entry `[e, i, l]` is 1 iff row i overlaps any row of layer l of
    `layers_1` by the rule above -- the `any(...)` that `ContactReward` and contact_rules.py:105 take.

The entry is for the ORDERED pair: row i is `self`, row j the argument.  matplotlib's parallel-segment branch measures from
the first path's end points and is not symmetric in general.  With `layers_1=None` the kernel fills `[j, i]` from `[i, j]` only
where the narrow phase proves the answer symmetric (a crossing of two non-parallel edges, or no parallel edge pair among
those tested); otherwise it evaluates both orders.

The predicate, on the record's float64 `position`, `_max_radius`, vertex count and world vertices:
    * `sqrt(fma(dy, dy, dx * dx)) > r0 + r1` gives 0 (numpy's 1-D norm of sprite.py:464);
    * otherwise it is `Path.intersects_path(a, b, filled=True)` as oracle/moog_oracle.c restates it: non-degenerate edges
      (squared length not `isclose` to 0) tested with matplotlib's `segments_intersect`, then both containment tests with the
      even-odd `point_in_path`;
    * a polygon without a finite vertex is an empty path and overlaps everything;
    * a vertex count above the slot's capacity is cut to the capacity.

No torus wrap-around and no polygon modifier: arena coordinates.

Refused, with a message: an unknown or repeated layer, an unknown mode, R0 or R1 of 0 or above MOOG_MAX_SLOTS, in 'layer'
mode a layer of `layers_1` without a sprite slot (its column could never be set), and a fifth `Contacts` in one config
(MOOG_MAX_CONTACTS = 4).  It works with or without renderers, beside tables, sensors and segmentations.
"""
import numpy as np

from .. import _abi
from .. import _dm_env as dm_env
from . import _rows

MODES = {'pair': _abi.MOOG_CONTACTS_PAIR, 'layer': _abi.MOOG_CONTACTS_LAYER}


def _layer_tuple(arg, what):
    if isinstance(arg, str):
        arg = (arg,)
    try:
        arg = tuple(arg)
    except TypeError:
        raise ValueError('Contacts: %s is a layer name or a tuple of names, got %r' % (what, arg))
    for name in arg:
        if not isinstance(name, str):
            raise ValueError('Contacts: %s is a layer name or a tuple of names, got %r' % (what, arg))
    return _rows.check_layers('Contacts', arg, what)


def contacts_layers(contacts):
    """Number of layers (runs of rows sharing a layer) in a lowered observer's second list; kept by lower()."""
    return int(contacts._n_layers_1)


def contacts_shape(contacts):
    """Per-env shape of a lowered observer (_abi.Contacts from Contacts.lower)."""
    if contacts.mode == _abi.MOOG_CONTACTS_LAYER:
        return (int(contacts.n_rows_0), contacts_layers(contacts))
    return (int(contacts.n_rows_0), int(contacts.n_rows_1))


def contacts_spec(contacts, name=None):
    return dm_env.specs.Array(shape=contacts_shape(contacts), dtype=np.uint8, name=name)


class Contacts(object):
    def __init__(self, layers_0, layers_1=None, mode='pair', visible_only=False):
        """See the module docstring."""
        self._layers_0 = _layer_tuple(layers_0, 'layers_0')
        self._layers_1 = None if layers_1 is None else _layer_tuple(layers_1, 'layers_1')
        if mode not in MODES:
            raise ValueError("Contacts: unknown mode %r (modes are 'pair' and 'layer')" % (mode,))
        self._mode, self._visible_only = mode, bool(visible_only)
        self._lowered = None   # the last lowering of this observer (compile_config), for observation_spec()

    @property
    def layers_0(self):
        return self._layers_0

    @property
    def layers_1(self):
        return self._layers_0 if self._layers_1 is None else self._layers_1

    @property
    def mode(self):
        return self._mode

    @property
    def visible_only(self):
        return self._visible_only

    def lower(self, program, layer_names):
        """(_abi.Contacts, (rows_0, rows_1)) of this observer over a lowered program: each rows list is [(layer name, index in
        layer)] per row, the rows of `SpriteTable(layers=...).lower`."""
        layer_names = list(layer_names)
        slots_0, rows_0 = _rows.layer_rows('Contacts', program, layer_names, self._layers_0, 'layers_0')
        slots_1, rows_1 = _rows.layer_rows('Contacts', program, layer_names, self.layers_1, 'layers_1')
        with_rows_1 = [name for name in self.layers_1 if (name, 0) in rows_1]
        if self._mode == 'layer':
            for name in self.layers_1:
                if name not in with_rows_1:
                    raise ValueError("Contacts: layer %r of layers_1 holds no sprite slot: its column of a mode='layer' tensor "
                                     'could never be set' % (name,))
        T = _abi.Contacts()
        T.n_rows_0, T.n_rows_1 = len(rows_0), len(rows_1)
        T.flags = _abi.MOOG_CONTACTS_VISIBLE_ONLY if self._visible_only else 0
        T.mode = MODES[self._mode]
        for k, s in enumerate(slots_0):
            T.row_slot_0[k] = s
        for k, s in enumerate(slots_1):
            T.row_slot_1[k] = s
        T._n_layers_1 = len(with_rows_1)
        self._lowered = T
        return T, (rows_0, rows_1)

    def observation_spec(self):
        """specs.Array((R0, R1) or (R0, n_layers_1), uint8): known once a config holding this observer has been lowered (an
        environment built from it, or _compiler.compile_config); `env.observation_spec()` always knows."""
        if self._lowered is None:
            raise ValueError('Contacts.observation_spec(): the row counts follow from the state_initializer and '
                             'layer_capacity -- build the environment first (env.observation_spec())')
        return contacts_spec(self._lowered)
