"""The collision response of the HIP step kernel against the recorded corpus of reference pairs
(tests/golden/collision_pairs.npz, tests/golden/make_golden.py make_collision_pairs): every pair is planted into an env of
its own, stepped once by the engine's physics, and compared with what the reference itself computed for it -- not with the
oracle, which tests/test_oracle_golden.py::test_collision_pairs_oracle holds to the same values at the same bar.
Needs an MI355X.

The programs step with the generic kernel (no specialised kernel is built for them; the specialised binaries are held equal
to the generic ones in tests/test_gpu_parity.py).  A case is one launch over a hundred envs of two sprites."""
import numpy as np
import pytest

import helpers
from test_gpu_parity import download, upload

pytestmark = pytest.mark.gpu
GROUPS = list(range(12))


def step_pairs(group, rows, monkeypatch):
    """The state records after one physics_step of pairs `rows` (pair rows[i] in env i) on the generic step kernel."""
    import torch  # noqa: F401
    from moog import environment
    monkeypatch.setenv('MOOG_STEP_SPEC', '0')
    fx = helpers.collision_pairs()
    env = environment.BatchedEnvironment(num_envs=len(rows), **helpers.pair_config(group))
    assert env.step_kernel() == 'generic', env.step_kernel()
    env.reset()
    f64, i32 = download(env)
    helpers.plant_pairs(env.compiled, f64, i32, fx, rows)
    upload(env, f64, i32)
    env.check_faults = False   # (the fault word is compared below, pair by pair)
    env.physics_step()
    f64, i32 = download(env)
    c = env.compiled
    env.close()
    return c, f64, i32


@pytest.mark.parametrize('group', GROUPS)
def test_collision_pairs_hip(group, monkeypatch):
    """pos / vel / angle / angvel of both sprites within 1e-9 (absolute) of the recorded reference values for every pair of
    the group, the float32 flags exact, no fault.  A failure names the pairs and the branches the reference took."""
    fx = helpers.collision_pairs()
    rows = helpers.pair_rows(group)
    c, f64, i32 = step_pairs(group, rows, monkeypatch)
    helpers.assert_pairs(c, f64, i32, fx, rows, 'engine')


def test_collision_pairs_hip_env_position_does_not_matter(monkeypatch):
    """Group 0 twice in one launch, the second half in reversed order: both halves bit-identical (and right)."""
    fx = helpers.collision_pairs()
    rows = helpers.pair_rows(0)
    n = len(rows)
    c, f64, i32 = step_pairs(0, np.concatenate([rows, rows[::-1]]), monkeypatch)
    helpers.assert_pairs(c, f64, i32, fx, rows, 'engine')
    assert np.array_equal(f64[:n].view(np.uint64), f64[n:][::-1].view(np.uint64)), 'float records depend on the env index'
    assert np.array_equal(i32[:n], i32[n:][::-1]), 'integer records depend on the env index'
