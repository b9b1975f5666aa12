"""Segmentation observer: per-pixel sprite ids of the rendered frame, drawn on the device.

The reference has frames (observers/pil_renderer.py) and the state itself (observers/raw_state.py), and leaves "which sprite
is visible at this pixel" to the caller.  Here that is an observer of its own: a `[num_envs, H, W]` uint8 tensor, rewritten in
place by every reset() / step() / observation() of a `BatchedEnvironment` on the calls that draw the frames
(include/moog_engine.h moog_engine_add_segmentation; csrc/moog_raster_mask_core.h rm_p5_ids).

What a pixel shows is defined through the reference's renderer: draw the state with `PILRenderer` (pil_renderer.py:100-118,
anti_aliasing 1, black background) with every polygon's colour replaced by (id, 0, 0) and its opacity by 255, leave out the
polygons of opacity 0, and take channel 0.  So coverage is Pillow's `ImageDraw.polygon` on the integer points the renderer
draws, the drawing order is the reference's (layers in state order, sprites in list order), rows are flipped as the frames'
are, and a mask and a frame of the same size and modifier align pixel for pixel.  A translucent sprite owns its pixels like
an opaque one; a sprite of opacity 0 owns none; 0 means no sprite.

mode='instance': id = 1 + row, rows being the sprite slots of the chosen layers, layer after layer -- the numbering of
`SpriteTable(layers=...)` rows, so mask value v is row v - 1 of a table over the same layers (`env.segmentation_rows(key)`
names the rows).  mode='layer': id = 1 + position of the sprite's layer in the chosen layers.  Sprites of layers that are not
chosen are still drawn and still occlude, and show as 0: the mask describes the frame the agent sees.
"""
import numpy as np

from .. import _abi
from .. import _dm_env as dm_env
from . import _rows
from . import polygon_modifiers

MODES = ('instance', 'layer')
MAX_SIDE = 128   # the mask rasteriser's frames (csrc/moog_raster_mask_core.h); larger ones are the span rasteriser's


def segmentation_spec(seg, name=None):
    """specs.Array((H, W), uint8) of a lowered segmentation (_abi.Segmentation)."""
    return dm_env.specs.Array(shape=(int(seg.height), int(seg.width)), dtype=np.uint8, name=name)


class Segmentation(object):
    def __init__(self, image_size=(64, 64), layers=None, mode='instance', polygon_modifier=None):
        """image_size: as PILRenderer's (a mask and a frame of the same image_size have the same height and width), each side
        at most 128.  layers: None (every layer of the state, in its order) or a tuple of layer names, used in the given
        order.  mode: 'instance' or 'layer'.  polygon_modifier: what PILRenderer accepts (DoNothing, TorusGeometry,
        FirstPersonAgent); a torus copy carries its sprite's id."""
        self._image_size = tuple(int(v) for v in image_size)
        if len(self._image_size) != 2 or min(self._image_size) < 1:
            raise ValueError('Segmentation: image_size must be two positive integers, got %r' % (image_size,))
        if max(self._image_size) > MAX_SIDE:
            raise NotImplementedError(
                'Segmentation: image_size %r -- frames above %d pixels a side are drawn by the span rasteriser, which has no '
                'id output; masks are available up to %d x %d' % (self._image_size, MAX_SIDE, MAX_SIDE, MAX_SIDE))
        if mode not in MODES:
            raise ValueError("Segmentation: unknown mode %r (modes are 'instance' and 'layer')" % (mode,))
        self._mode = mode
        self._layers = None if layers is None else _rows.check_layers('Segmentation', layers)
        if polygon_modifier is None:
            polygon_modifier = polygon_modifiers.DoNothing()
        if not isinstance(polygon_modifier, (polygon_modifiers.DoNothing, polygon_modifiers.TorusGeometry,
                                             polygon_modifiers.FirstPersonAgent)):
            raise NotImplementedError('Segmentation: polygon modifier %r' % (type(polygon_modifier).__name__,))
        self._polygon_modifier = polygon_modifier

    @property
    def layers(self):
        return self._layers

    @property
    def mode(self):
        return self._mode

    @property
    def polygon_modifier(self):
        return self._polygon_modifier

    def lower(self, program, layer_names):
        """(_abi.Segmentation, [(layer name, index in layer)] per row) of this observer over a lowered program: the rows are
        `SpriteTable(layers=...).lower`'s; slot_id[s] is what sprite slot s shows as."""
        layer_names = list(layer_names)
        names = layer_names if self._layers is None else list(self._layers)
        G = _abi.Segmentation()
        G.width, G.height = self._image_size   # (PILRenderer's convention: image_size[0] scales x)
        G.n_slots = int(program.n_slots)
        pm = self._polygon_modifier
        if isinstance(pm, polygon_modifiers.TorusGeometry):
            G.polymod = _abi.MOOG_POLYMOD_TORUS
        elif isinstance(pm, polygon_modifiers.FirstPersonAgent):
            if pm._agent_layer not in layer_names:
                raise ValueError('Segmentation: unknown agent layer %r (the state has %s)'
                                 % (pm._agent_layer, ', '.join(layer_names)))
            G.polymod, G.polymod_layer = _abi.MOOG_POLYMOD_FIRST_PERSON, layer_names.index(pm._agent_layer)
        else:
            G.polymod = _abi.MOOG_POLYMOD_NONE
        slots, rows = _rows.layer_rows('Segmentation', program, layer_names, self._layers)
        if self._mode == 'instance' and len(rows) > 255:
            raise NotImplementedError(
                'Segmentation: more than 255 rows in instance mode (an id is one byte, 0 is "no sprite"): '
                "choose fewer layers, or mode='layer'")
        for r, (s, (name, _)) in enumerate(zip(slots, rows)):
            G.slot_id[s] = 1 + r if self._mode == 'instance' else 1 + names.index(name)
        return G, rows

    def observation_spec(self):
        """specs.Array((H, W), uint8)."""
        return dm_env.specs.Array(shape=(self._image_size[1], self._image_size[0]), dtype=np.uint8)
