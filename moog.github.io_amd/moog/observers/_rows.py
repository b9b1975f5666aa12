"""What the device observers share when they are lowered: the row list over chosen layers, the check of a layer tuple and
the float32 / float16 dtype table.

A row list is the sprite slots of the chosen layers, layer after layer, numbered as a `SpriteTable` numbers them: row r of a
`SpriteTable(layers=L)` is row r (id r + 1) of a `RaySensor`, a `Segmentation` or a `Contacts` argument over the same L.
"""
import numpy as np

from .. import _abi

# dtype name -> MOOG_TABLE_* (include/moog_engine.h): what a SpriteTable and a RaySensor can be written as
DTYPES = {'float32': _abi.MOOG_TABLE_F32, 'float16': _abi.MOOG_TABLE_F16}


def check_dtype(who, dtype):
    """The name of `dtype` when it is one of DTYPES; `who` is the observer's class name."""
    try:
        name = np.dtype(dtype).name
    except TypeError:
        name = None
    if name not in DTYPES:
        raise ValueError("%s: dtype must be 'float32' or 'float16', got %r" % (who, dtype))
    return name


def numpy_dtype(code):
    """numpy dtype of a MOOG_TABLE_* code."""
    return np.dtype(np.float16 if code == _abi.MOOG_TABLE_F16 else np.float32)


def check_layers(who, layers, what='layers'):
    """`layers` (argument `what` of observer `who`) as a tuple: a tuple of names, not one string, and no name twice."""
    if isinstance(layers, str):
        raise ValueError('%s: %s is a tuple of names, not one string' % (who, what))
    layers = tuple(layers)
    if len(set(layers)) != len(layers):
        raise ValueError('%s: a layer is named twice in %s=%r' % (who, what, layers))
    return layers


def layer_rows(who, program, layer_names, names=None, what=None):
    """([slot], [(layer name, index in layer)]) per row over the layers `names` (None: every layer of the state, in its order)
    of a lowered program.  `who` is the observer's class name; `what`, where the observer takes more than one layer argument,
    the argument's name."""
    layer_names = list(layer_names)
    where = ' in %s' % what if what else ''
    slots, rows = [], []
    for name in (layer_names if names is None else names):
        if name not in layer_names:
            raise ValueError('%s: unknown layer %r%s (the state has %s)' % (who, name, where, ', '.join(layer_names)))
        li = layer_names.index(name)
        s0, n = int(program.layer_slot0[li]), int(program.layer_nslots[li])
        slots.extend(range(s0, s0 + n))
        rows.extend((name, k) for k in range(n))
    if not rows:
        raise ValueError('%s: the layers of %s hold no sprite slot (0 rows)' % (who, what or 'the chosen layers'))
    if len(rows) > _abi.MOOG_MAX_SLOTS:
        raise ValueError('%s: more than %d rows%s (MOOG_MAX_SLOTS), got %d' % (who, _abi.MOOG_MAX_SLOTS, where, len(rows)))
    return slots, rows
