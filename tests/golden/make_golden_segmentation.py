"""Generates the golden vectors of the Segmentation observer (seg_zoo) from the REAL reference.

Run in the build container only (needs /root/reference, matplotlib, Pillow), like make_golden_views.py:

    PYTHONPATH=oracle/shim:/root/reference MPLBACKEND=Agg python tests/golden/make_golden_segmentation.py

The reference has no segmentation observer.  What one shows is defined through the reference's own, unmodified PILRenderer
(moog/observers/pil_renderer.py:88-120; anti_aliasing 1, identity colour map, black background) fed by a polygon modifier of
ours that wraps the config's: every polygon keeps its vertices, its colour becomes (id, 0, 0), its opacity 255, and
polygons of opacity 0 are left out (Pillow's blend leaves their pixels untouched).  Channel 0 of what the renderer returns is
the mask.  make_golden.record_config records the calls as for every other recording; the masks of every Segmentation key of
the level (seg_zoo.segmentations) are added as `ids_<key>` [calls, H, W] uint8, one per recorded call.

The files are named seg_zoo_l<level>.npz -- without the `_s<seed>` of the recordings helpers.RUNS lists: they have tests of
their own (tests/test_segmentation_*.py).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402  (patch_numpy_random, record_config, load_amd_config)
import make_golden_views  # noqa: E402  (RecordingRenderer)
from moog.observers import pil_renderer as ref_pil  # noqa: E402  (the reference package)
from moog.observers import polygon_modifiers as ref_pm  # noqa: E402


class IdModifier(ref_pm.AbstractPolygonModifier):
    """The config's polygon modifier with every polygon recoloured to its sprite's id."""

    def __init__(self, inner, layers, mode, caps):
        self._inner, self._layers, self._mode, self._caps = inner, layers, mode, caps

    def __call__(self, state):
        inner = self._inner(state)
        names = list(state.keys()) if self._layers is None else list(self._layers)
        ids, row0 = {}, 0
        for pos, name in enumerate(names):   # rows: the slots of the chosen layers, layer after layer (capacity slots each)
            for k, s in enumerate(state[name]):
                ids[id(s)] = 1 + row0 + k if self._mode == 'instance' else 1 + pos
            row0 += self._caps.get(name, len(state[name]))

        def recoloured(layer, sprite):
            return [(vertices, (ids.get(id(sprite), 0), 0, 0), 255)
                    for vertices, _, opacity in inner(layer, sprite) if opacity != 0]
        return recoloured


# (level, calls, make_golden.record_config options)
PLAN = [(0, 40, {}), (1, 40, {}), (2, 40, {}), (3, 24, {'__vmax__': make_golden.SNAP_VMAX}),
        (4, 40, {'prey': 8, 'predators': 8, '__dynamic__': ('prey', 'predators')})]


def main():
    make_golden.patch_numpy_random()
    for level, n_calls, options in PLAN:
        name = 'seg_zoo_l%d' % level
        cfg = make_golden.load_amd_config(name)
        seg_zoo = sys.modules['amd_configs.seg_zoo']   # (load_amd_config imports this repo's recipes as `amd_configs`)
        caps = {k: v for k, v in options.items() if not k.startswith('__')}
        recorders = {}
        for key, kw in seg_zoo.segmentations(level).items():
            inner = cfg['observers']['image'].polygon_modifier
            renderer = ref_pil.PILRenderer(image_size=kw['image_size'], anti_aliasing=1,
                                           polygon_modifier=IdModifier(inner, kw['layers'], kw['mode'], caps))
            recorders[key] = cfg['observers']['ids_' + key] = make_golden_views.RecordingRenderer(renderer)
        make_golden.record_config(name, cfg, 0, n_calls, dict(options))
        recorded = os.path.join(HERE, '%s_s0.npz' % name)
        data = dict(np.load(recorded))
        os.remove(recorded)
        for key, rec in recorders.items():
            frames = np.stack(rec.frames)
            assert frames.shape[0] == n_calls + 1, (key, frames.shape)
            assert not frames[..., 1:].any()
            data['ids_' + key] = np.ascontiguousarray(frames[..., 0])
        path = os.path.join(HERE, '%s.npz' % name)
        np.savez_compressed(path, **data)
        print('%-14s %s  %.0f KB' % (name, ', '.join('%s %s max id %d' % (k, data['ids_' + k].shape[1:], data['ids_' + k].max())
                                                      for k in recorders), os.path.getsize(path) / 1024.))


if __name__ == '__main__':
    main()
