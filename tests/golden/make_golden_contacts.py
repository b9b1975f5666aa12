"""Generates the golden vectors of the Contacts observer: who overlaps whom in every recorded call of four recordings.

Run by hand where matplotlib is (40 to 220 s per recording), like make_golden_segmentation.py; no test runs it:

    MPLBACKEND=Agg python tests/golden/make_golden_contacts.py

This script does NOT re-run the reference's episodes.  It applies the reference's predicate -- sprite.py:462-484
`Sprite.overlaps_sprite`: `np.linalg.norm(p0 - p1) > r0 + r1` gives False, else matplotlib's
`Path.intersects_path(a.path, b.path, filled=True)` over the closed paths (the vertices plus the first one again) -- to the
state the recording already holds for every call: `pos`, `maxr`, `nverts`, `verts` and `alive` of
tests/golden/<name>_s0.npz, which make_golden.py recorded from the reference's own sprites.

For each recording it writes tests/golden/contacts_<name>_s0.npz:
    bits    uint8 [calls, ceil(S * S / 8)]: np.packbits of the [S, S] matrix m[a, b] = a.overlaps_sprite(b) over every ordered
            pair of distinct live sprite slots (0 elsewhere), one row per recorded call;
    n_slots S;
    counts  int64 [3]: ordered live pairs, pairs past the bounding-circle test, overlapping pairs, summed over the calls.
The counts must equal the ones measured when the observer was specified (EXPECT below).
"""
import os
import sys

import numpy as np
from matplotlib import path as mpl_path

HERE = os.path.dirname(os.path.abspath(__file__))

# recording: (calls, ordered live pairs, past the circle, overlapping)
EXPECT = {
    'colliding_predators_32': (41, 40672, 4542, 446),
    'falling_balls_64': (13, 52416, 2612, 78),
    'cleanup': (151, 140430, 12820, 2308),
    'pong': (97, 1812, 1394, 436),
}


def contacts_of(fx):
    """([calls, S, S] uint8, (live pairs, past the circle, overlapping)) of a recording."""
    calls, S = fx['alive'].shape[0], fx['alive'].shape[1]
    out = np.zeros((calls, S, S), np.uint8)
    n_pairs = n_circle = n_hit = 0
    for t in range(calls):
        live = [s for s in range(S) if fx['alive'][t][s]]
        paths = {}
        for s in live:
            v = np.asarray(fx['verts'][t][s, :int(fx['nverts'][t][s])], np.float64)
            paths[s] = mpl_path.Path(np.concatenate([v, v[:1]], axis=0))
        for a in live:
            pa, ra = np.asarray(fx['pos'][t][a], np.float64), float(fx['maxr'][t][a])
            for b in live:
                if a == b:
                    continue
                n_pairs += 1
                pb, rb = np.asarray(fx['pos'][t][b], np.float64), float(fx['maxr'][t][b])
                if np.linalg.norm(pa - pb) > ra + rb:
                    continue
                n_circle += 1
                if mpl_path.Path.intersects_path(paths[a], paths[b], filled=True):
                    out[t, a, b] = 1
                    n_hit += 1
    return out, (n_pairs, n_circle, n_hit)


def main(names):
    for name in names:
        with np.load(os.path.join(HERE, '%s_s0.npz' % name)) as z:
            fx = {k: z[k] for k in ('alive', 'pos', 'maxr', 'nverts', 'verts')}
        m, counts = contacts_of(fx)
        got = (m.shape[0],) + counts
        print('%-26s calls %d, ordered live pairs %d, past the circle %d, overlapping %d' % ((name,) + got))
        assert got == EXPECT[name], (name, got, EXPECT[name])
        np.savez_compressed(os.path.join(HERE, 'contacts_%s_s0.npz' % name),
                            bits=np.packbits(m.reshape(m.shape[0], -1), axis=1), n_slots=np.int64(m.shape[1]),
                            counts=np.array(counts, np.int64))


if __name__ == '__main__':
    main(sys.argv[1:] or list(EXPECT))
