"""Generates reference_programs.npz: the lowered program (moog._abi.Program, as bytes) of every config file of the
reference that tests/test_host.py::test_reference_configs_load_unchanged pins.

    python tests/golden/make_reference_programs.py <reference checkout>

The reference's own config files (<reference checkout>/moog_demos/example_configs/<name>.py) are executed unmodified
against this repository's `moog` and lowered by its compiler; the test compares the stored bytes with the lowering of
the re-stated recipes in moog_demos/example_configs, so it needs no reference checkout.  Keys: '<name>_l<level>'.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.normpath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, os.path.join(REPO, 'moog.github.io_amd'))

# (config, level): the cases of test_reference_configs_load_unchanged
CASES = [('pong', 0), ('chase_avoid_torus', 0), ('colliding_predators', 0), ('functional_maze', 0), ('falling_balls', 0),
         ('first_person_predators_prey', 0), ('cleanup', 0), ('pacman', 0), ('pacman', 1), ('parallelogram_catch', 0),
         ('parallelogram_catch', 2), ('multi_tracking_with_feature', 3), ('match_to_sample', 2), ('match_to_sample', 3),
         ('match_to_sample', 4), ('predators_arena', 1), ('predators_arena', 2), ('predators_arena', 3),
         ('bounce_box_contact_prediction', 0), ('bounce_box_contact_prediction', 1), ('red_green', 0), ('red_green', 1),
         ('red_green', 2), ('red_green', 3)]


def key(name, level):
    return '%s_l%d' % (name, level)


def main(ref):
    from moog import _compiler
    from moog_demos import example_configs
    configs = os.path.join(ref, 'moog_demos', 'example_configs')
    out = {}
    for name, level in CASES:
        spec = importlib.util.spec_from_file_location('ref_' + name, os.path.join(configs, name + '.py'))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        c = _compiler.compile_config(layer_capacity=example_configs.capacity(name), **m.get_config(level))
        out[key(name, level)] = np.frombuffer(bytes(c.program), np.uint8)
    path = os.path.join(HERE, 'reference_programs.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d programs)' % (path, len(out)))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
