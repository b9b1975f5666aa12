"""Generates the golden vectors of configs with several observers (views_zoo) from the REAL reference.

Run in the build container only (needs /root/reference, matplotlib, Pillow), like make_golden.py:

    PYTHONPATH=oracle/shim:/root/reference MPLBACKEND=Agg python tests/golden/make_golden_views.py

The reference's Environment.observation() returns {key: observer(state)} for every observer of the config
(moog/environment.py:128-131).  make_golden.record_config records the calls (per-call sprite tables, bookkeeping, the
uniforms each call consumed, the 'image' frames); here every PILRenderer of the config is replaced by a recording
subclass that keeps each frame it draws, and the frames of every renderer key are added to the file as `image_<key>`
[calls, H, W, 3] (one frame per recorded call: reset, then every step).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402  (Tape, patch_numpy_random, record_config, load_amd_config)
from moog.observers import pil_renderer as ref_pil  # noqa: E402  (the reference package)


class RecordingRenderer(ref_pil.PILRenderer):
    """The reference's PILRenderer, keeping a copy of every frame it returns."""

    def __init__(self, src):   # (a copy of an existing renderer: same settings, same drawing code)
        self.__dict__.update(src.__dict__)
        self.frames = []

    def __call__(self, state):
        img = super(RecordingRenderer, self).__call__(state)
        self.frames.append(np.array(img, copy=True))
        return img


# (level, calls): few calls for l2, whose 256 x 256 frames keep the file under 1 MB
PLAN = [(0, 40), (1, 40), (2, 8)]


def main():
    make_golden.patch_numpy_random()
    for level, n_calls in PLAN:
        name = 'views_zoo_l%d' % level
        cfg = make_golden.load_amd_config(name)
        recorders = {}
        obs = {}
        for key, o in cfg['observers'].items():
            if isinstance(o, ref_pil.PILRenderer):
                o = recorders[key] = RecordingRenderer(o)
            obs[key] = o
        cfg['observers'] = obs
        make_golden.record_config(name, cfg, 0, n_calls, {})
        path = os.path.join(HERE, '%s_s0.npz' % name)
        data = dict(np.load(path))
        for key, rec in recorders.items():
            frames = np.stack(rec.frames)
            assert frames.shape[0] == n_calls + 1, (key, frames.shape)
            data['image_' + key] = frames
        np.savez_compressed(path, **data)
        print('%-26s views %s  %.0f KB' % (name, ', '.join('%s %s' % (k, data['image_' + k].shape[1:3]) for k in recorders),
                                           os.path.getsize(path) / 1024.))


if __name__ == '__main__':
    main()
