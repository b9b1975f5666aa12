"""CPU-only checks of the host side: config lowering, ABI symbols, layout."""
import ctypes
import os

import numpy as np
import pytest

import helpers
from moog import _abi, _compiler, _engine
from moog_demos import example_configs

PKG = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'moog.github.io_amd')


def test_layout_matches_header():
    """Python layout_of() == the header's moog_layout() (as compiled into the oracle)."""
    for name in example_configs.NAMES:
        c = helpers.compiled(name)
        L = c.layout
        assert L.f64_per_env % 2 == 0 and L.i32_per_env % 4 == 0
        o = helpers.OracleEnv(c)
        assert o.f64.shape[1] == L.f64_per_env
    assert helpers.oracle().oracle_program_sizeof() == ctypes.sizeof(_abi.Program)


def test_runs_list_equals_the_recordings_on_disk():
    """helpers.RUNS -- the list the oracle tests and the HIP tests are parametrised by -- names every reference recording
    in tests/golden and nothing else: a recording that is on disk but not in the list (or the other way round) would be
    untested without anybody noticing.  The recordings with a test of their own are named in helpers, one by one."""
    runs = list(helpers.RUNS)
    assert len(set(runs)) == len(runs), 'an entry twice: %s' % sorted(r for r in set(runs) if runs.count(r) > 1)
    disk = helpers.recordings_on_disk()
    own = set(helpers.RECORDINGS_WITH_OWN_TESTS)
    assert own <= set(disk), 'named as tested elsewhere but not on disk: %s' % sorted(own - set(disk))
    assert not own & set(runs)
    assert set(disk) - own == set(runs), ('on disk but not in RUNS: %s; in RUNS but not on disk: %s' % (
        sorted(set(disk) - own - set(runs)), sorted(set(runs) - set(disk))))
    # the recordings whose call 0 is no reset are the ones the reset-sampler test leaves out, and no others
    mid = sorted(r for r in runs if int(helpers.fixture(*r)['step_type'][0]) != 0)
    assert mid == sorted(helpers.MID_EPISODE_RUNS), mid
    # every program BASELINE.json measures has recordings, and they are the programs build() specialises a step kernel for
    import __graft_entry__ as entry
    assert sorted(helpers.BASELINE_PROGRAMS) == sorted(entry.SPEC_WORKLOADS)
    for name in helpers.BASELINE_PROGRAMS:
        assert any(r[0] == name for r in runs), name


def test_hip_library_exports_abi():
    """The C-ABI library loads and exports every symbol include/moog_engine.h declares."""
    lib = _engine.load_library()
    for sym in _engine.SYMBOLS:
        assert hasattr(lib, sym), sym
    assert lib.moog_abi_version() == _abi.MOOG_ABI_VERSION
    assert lib.moog_program_sizeof() == ctypes.sizeof(_abi.Program)
    import re
    hdr = open(_abi.HEADER).read()
    declared = set(re.findall(r'\b(moog_\w+)\s*\(', hdr)) - {'moog_layout', 'moog_align_'}
    assert declared == set(_engine.SYMBOLS), declared ^ set(_engine.SYMBOLS)


def test_built_objects_carry_the_source_digest():
    """moog/_digest.py: libmoog_hip.so and every specialised step kernel in lib/spec carry the digest of the kernel sources
    and flags they were built from; __graft_entry__.build() leaves no object of another build behind (the engine would refuse
    it one by one: csrc/moog_engine.hip load_spec_kernel, tests/test_gpu_parity.py::test_specialised_kernel_of_another_build_is_refused)."""
    import glob
    from moog import _digest, _spec
    d = _digest.source_digest()
    assert len(d) == 16 and _digest.digest_of(_engine.LIB_PATH) == d, 'libmoog_hip.so is not the build of these sources: run __graft_entry__.build()'
    assert '%016x' % _engine.load_library().moog_source_digest() == d
    objs = sorted(glob.glob(os.path.join(_spec.SPEC_DIR, 'step_*.so')))
    assert len(objs) >= 4, 'the BASELINE workloads\' specialised kernels are built by __graft_entry__.build()'
    stale = [os.path.basename(o) for o in objs if not _spec.is_current(o, d)]
    assert not stale, stale
    assert _digest.digest_of(os.path.join(_spec.SPEC_DIR, 'no_such_object.so')) is None


def test_step_kernels_have_no_calls(tmp_path):
    """Every device function is inlined into the step / reset kernels: the env's descriptor (`Env`, moog_device.h) lives in
    registers only then.  One function left out of line takes it by reference through scratch memory (round 4: the step
    kernel at 1270 us instead of 800 the day the inliner left apply_physics out).  Checks the built objects' gfx950 code."""
    import glob
    import subprocess
    llvm = '/opt/rocm/lib/llvm/bin'
    # (the variants that carry every component -- m3 / m4, the full reset kernel -- are beyond the inliner: their rarely used
    #  paths stay calls, and their programs pay for it)
    objs = sorted(glob.glob(os.path.join(PKG, 'lib', 'moog_step_[ft]*.o')) + glob.glob(os.path.join(PKG, 'lib', 'moog_reset_r0.o')))
    if not objs or not os.path.exists(os.path.join(llvm, 'llvm-objdump')):
        pytest.skip('no built step objects / no llvm tools here')
    for o in objs:
        fat, co = str(tmp_path / 'fat.bin'), str(tmp_path / 'dev.co')
        subprocess.check_call([os.path.join(llvm, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, o, str(tmp_path / 'scratch.o')])
        subprocess.check_call([os.path.join(llvm, 'clang-offload-bundler'), '--unbundle', '--type=o',
                               '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + fat, '--output=' + co])
        asm = subprocess.check_output([os.path.join(llvm, 'llvm-objdump'), '-d', co]).decode()
        assert 's_swappc_b64' not in asm, '%s: a device function was not inlined' % os.path.basename(o)


def _kernel_notes(path, tmp_path):
    """[(kernel name, private segment bytes, spilled VGPRs, spilled SGPRs, VGPRs)] of a host object / shared library's first gfx950 code object."""
    import re
    import subprocess
    llvm = '/opt/rocm/lib/llvm/bin'
    fat, co = str(tmp_path / 'fat.bin'), str(tmp_path / 'dev.co')
    subprocess.check_call([os.path.join(llvm, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, path, str(tmp_path / 'scratch.o')])
    subprocess.check_call([os.path.join(llvm, 'clang-offload-bundler'), '--unbundle', '--type=o',
                           '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + fat, '--output=' + co])
    notes = subprocess.check_output([os.path.join(llvm, 'llvm-readelf'), '--notes', co]).decode()
    out = []
    for block in notes.split('  - .agpr_count')[1:]:
        g = lambda k: int(re.search(r'\.' + k + r':\s+(\d+)', block).group(1))
        out.append((re.search(r'\.name:\s+(\S+)', block).group(1), g('private_segment_fixed_size'), g('vgpr_spill_count'), g('sgpr_spill_count'), g('vgpr_count')))
    return out


def test_kernel_scratch_report(tmp_path, capsys):
    """VERDICT r04 item 3 asked for the scratch of every kernel on record and for none in the plain step kernel.  The report is
    printed (pytest -s) and bounded here so that a regression shows: the plain generic kernel f3 and the specialised kernel of
    the headline workload keep their frames small (the live state of the collision recursion at three waves per SIMD: 168
    registers), the mask rasteriser spills nothing, and nothing uses more than the every-component variants' frames."""
    import glob
    if not os.path.exists('/opt/rocm/lib/llvm/bin/llvm-readelf'):
        pytest.skip('no llvm tools here')
    objs = sorted(glob.glob(os.path.join(PKG, 'lib', 'moog_step_*.o')) + glob.glob(os.path.join(PKG, 'lib', 'moog_reset_r*.o')) +
                  [os.path.join(PKG, 'lib', 'moog_raster.o')] + glob.glob(os.path.join(PKG, 'lib', 'spec', 'step_417c47560f31861d_*.so')))
    objs = [o for o in objs if os.path.exists(o)]
    if not objs:
        pytest.skip('no built objects')
    rows = []
    for o in objs:
        for name, priv, vs, ss, vg in _kernel_notes(o, tmp_path):
            rows.append((os.path.basename(o), name, priv, vs, ss, vg))
    with capsys.disabled():
        for r in rows:
            print('%-34s %-52s scratch %5d B  spilled VGPRs %4d  SGPRs %5d  VGPRs %3d' % r)
    by = {(r[0], r[1]): r for r in rows}
    for (obj, name), r in by.items():
        if 'raster_mask_kernel' in name:
            assert r[3] == 0, (obj, name, 'the mask rasteriser spills vector registers')
        if obj.startswith('moog_step_f3') and 'step_kernel' in name:
            assert r[2] <= 160 and r[3] <= 48, (obj, name, r)
        if obj.startswith('step_417c') and 'step_kernel' in name:
            assert r[2] <= 128 and r[3] <= 40, (obj, name, r)
        assert r[2] <= 4096, (obj, name, r)


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(_engine.EngineError):
        _engine.load_library(str(tmp_path / 'nope.so'))


@pytest.mark.parametrize('name,level', [('pong', 0), ('chase_avoid_torus', 0), ('colliding_predators', 0),
                                        ('functional_maze', 0), ('falling_balls', 0),
                                        ('first_person_predators_prey', 0), ('cleanup', 0), ('pacman', 0),
                                        ('pacman', 1), ('parallelogram_catch', 0), ('parallelogram_catch', 2),
                                        ('multi_tracking_with_feature', 3), ('match_to_sample', 2),
                                        ('match_to_sample', 3), ('match_to_sample', 4), ('predators_arena', 1),
                                        ('predators_arena', 2), ('predators_arena', 3),
                                        ('bounce_box_contact_prediction', 0), ('bounce_box_contact_prediction', 1),
                                        ('red_green', 0), ('red_green', 1), ('red_green', 2), ('red_green', 3)])
def test_reference_configs_load_unchanged(name, level):
    """The reference's own config files import this repo's `moog` and lower to the
    same program as the re-stated recipes.  The programs they lower to are stored in
    tests/golden/reference_programs.npz (tests/golden/make_reference_programs.py)."""
    with np.load(os.path.join(helpers.GOLDEN, 'reference_programs.npz')) as g:
        ref = g['%s_l%d' % (name, level)].tobytes()
    mine = helpers.compiled(name if level == 0 else '%s_l%d' % (name, level))
    assert ref == bytes(mine.program)


def test_program_contents():
    c = helpers.compiled('colliding_predators_32')
    P = c.program
    assert P.n_slots == 32 and c.layer_names == ['walls', 'predators', 'agent']
    assert P.updates_per_env_step == 10 and P.n_forces == 4
    kinds = [P.forces[i].kind for i in range(4)]
    assert kinds == [_abi.MOOG_FORCE_DRAG] + [_abi.MOOG_FORCE_COLLISION] * 3
    assert [P.forces[i].symmetric for i in range(1, 4)] == [1, 0, 0]
    assert P.timeout_steps == 200
    c = helpers.compiled('pong')
    T = c.program.tasks[1]
    assert (T.kind, T.cond, T.cond_value) == (_abi.MOOG_TASK_RESET, _abi.MOOG_COND_ALL_Y_LT, 0.0)
    assert c.layer_names[T.cond_layer] == 'prey'
    c = helpers.compiled('functional_maze')
    assert [c.program.rules[i].kind for i in range(3)] == [
        _abi.MOOG_RULE_VANISH_ON_CONTACT, _abi.MOOG_RULE_PORTAL, _abi.MOOG_RULE_BOOSTER]
    prey = c.program.ops[c.program.n_ops - 1]
    assert (prey.count_min, prey.count_max) == (2, 4)


def test_unsupported_components_raise():
    from moog import game_rules, observers, tasks, physics
    # lowered since round 4 (tests/golden/callables_zoo*.npz pin them against the reference)
    tasks.ContactReward(1., 'a', 'b', condition=lambda a, b, meta_state: meta_state['phase'] == 'go')
    assert physics.DistanceForce(lambda d: 0.1 * d if d < 1 else 0.)._force_node is not None
    assert game_rules.DelayedRule(lambda: np.random.randint(2, 5), ())._random == (1, 2.0, np.inf, 5.0)
    # any Python colour function: evaluated on the host per distinct colour (tests/golden/callables_zoo_l2_s0.npz)
    assert observers.PILRenderer(image_size=(8, 8), color_to_rgb=lambda c: (int(c[0]), 0, 0))._cmap == 'callable'
    assert observers.PILRenderer(image_size=(8, 8), color_to_rgb='hsv_to_rgb')._cmap == 'hsv'
    from moog import environment
    call = environment.BatchedEnvironment._call_color_fn
    assert call(lambda c: (300, int(64 * c[1]), -20), (0.9, 1.0, 1.0)) == 255 | (64 << 8)   # Pillow clips the ink
    assert call(lambda c: c, (255.0, 128.0, 0.0)) == 255 | (128 << 8)                       # integral components arrive as ints
    with pytest.raises(TypeError):
        call(lambda c: (0.5, 0, 0), (0.1, 0.2, 0.3))                                        # Pillow takes integers only
    # still refused, with a message: what the tracer cannot follow
    with pytest.raises(NotImplementedError):
        physics.DistanceForce(lambda d: float(d) ** 2)            # float() of a traced value
    with pytest.raises(NotImplementedError):
        game_rules.TimedRule(lambda: (np.random.randint(0, 3), np.random.randint(5, 9)), ())   # two draws
    with pytest.raises(NotImplementedError):
        tasks.Reset(condition=lambda state: len(state['x']) > 3).classify(['x', 'y'])


def test_shape_table_matches_reference_fixture():
    """Host-side shape records (centroid shift, inertia) reproduce the reference's
    sprites: the reset of every fixture already pins them (test_oracle_golden),
    here the unit-area property of the named shapes is checked directly."""
    from moog import shapes
    for name, v in shapes.SHAPES.items():
        x, y = v[:, 0], v[:, 1]
        area = 0.5 * np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)
        assert abs(area - 1.0) < 1e-12, name


def test_meta_state_rules_stay_on_the_host():
    """ModifyMetaState (modify_meta_state.py:7-24) never touches sprites: the lowering skips
    it and accepts a meta_state_initializer (environment.py:60-63)."""
    import collections
    from moog import _compiler, action_spaces, game_rules, observers, physics as physics_lib
    from moog import sprite, tasks
    bump = game_rules.ModifyMetaState(lambda m: m.__setitem__('key', m['key'] + 1))
    c = _compiler.compile_config(
        state_initializer=lambda: collections.OrderedDict(
            [('agent', [sprite.Sprite(x=0.5, y=0.5, scale=0.1, c0=128)])]),
        physics=physics_lib.Physics(),
        task=tasks.ContactReward(1., 'agent', 'agent'),
        action_space=action_spaces.Grid(0.1, action_layers='agent', control_velocity=True),
        observers={'image': observers.PILRenderer(image_size=(64, 64))},
        game_rules=(bump,), meta_state_initializer=lambda: {'key': 0})
    assert c.program.n_rules == 0
    m = {'key': 0}
    bump.step(None, m)
    assert m['key'] == 1


def test_composite_distributions_lower_to_programs():
    """Mixture / Intersection / SetMinus / Selection / Discrete(probs) become distribution
    programs (include/moog_engine.h moog_dinstr_t); flat Products keep the per-factor path."""
    from moog import _abi
    from moog.state_initialization import distributions as distribs
    c = helpers.compiled('distrib_zoo')
    P = c.program
    tree_ops = [P.ops[i] for i in range(P.n_ops) if P.ops[i].code_off >= 0]
    assert len(tree_ops) == 2 and P.n_dcode > 20
    ops = [P.dcode[i].op for i in range(P.n_dcode)]
    for need in (_abi.MOOG_D_CHOICE, _abi.MOOG_D_LOOP, _abi.MOOG_D_TEST, _abi.MOOG_D_DISCP,
                 _abi.MOOG_P_RANGE, _abi.MOOG_P_AND, _abi.MOOG_P_OR, _abi.MOOG_D_END):
        assert need in ops
    for i in range(P.n_dcode):       # every jump / loop target stays inside the table
        I = P.dcode[i]
        if I.op == _abi.MOOG_D_JUMP:
            assert 0 <= I.a < P.n_dcode
        if I.op == _abi.MOOG_D_TEST:
            assert 0 <= int(I.x) < i and I.c + I.b <= P.n_dcode
    assert all(helpers.compiled('colliding_predators').program.ops[i].code_off == -1
               for i in range(helpers.compiled('colliding_predators').program.n_ops))
    # outside a traced initializer the classes sample with numpy, by the reference's algorithm
    d = distribs.SetMinus(distribs.Continuous('x', 0., 1.), distribs.Continuous('x', 0.2, 0.9))
    xs = [float(d.sample()['x']) for _ in range(50)]
    assert all((0. <= x < 0.2) or (0.9 <= x < 1.) for x in xs)
    m = distribs.Mixture([distribs.Discrete('k', [1]), distribs.Discrete('k', [2])], probs=[0., 1.])
    assert m.sample()['k'] == 2 and m.contains({'k': 1}) and not m.contains({'k': 3})


def test_config_callables_are_traced_symbolically():
    """Sprite filters / modifiers / pair functions (e.g. cleanup.py:150-216,
    first_person_predators_prey.py:129-147,193-201) run once on symbolic sprites; Python
    control flow is covered by enumerating the execution paths."""
    from moog import _symbolic as sy
    lo, hi = -1.2, 2.2

    def should_vanish(s):
        too_small = (s.position < lo) * (s.velocity < 0.)
        too_large = (s.position > hi) * (s.velocity > 0.)
        return any(too_small) or any(too_large)
    code = sy.emit(sy.trace_value(should_vanish, 1), [])
    assert sy.depth(code) <= _abi.MOOG_X_STACK

    def evaluate(code, attrs):   # reference evaluator of the postfix code, Python floats
        st = []
        for ins in code:
            op = ins['op']
            if op == _abi.MOOG_X_CONST:
                st.append(ins['x'])
            elif op == _abi.MOOG_X_ATTR:
                st.append(attrs[ins['b']][sy.ATTRS[ins['a']]])
            elif op == _abi.MOOG_X_SELECT:
                b, a, c = st.pop(), st.pop(), st.pop()
                st.append(a if c else b)
            elif op == _abi.MOOG_X_MUL:
                b, a = st.pop(), st.pop(); st.append(a * b)
            elif op == _abi.MOOG_X_LT:
                b, a = st.pop(), st.pop(); st.append(float(a < b))
            elif op == _abi.MOOG_X_GT:
                b, a = st.pop(), st.pop(); st.append(float(a > b))
            else:
                raise AssertionError(op)
        return st[-1]

    class S(object):
        def __init__(self, x, y, vx, vy):
            self.position, self.velocity = np.array([x, y]), np.array([vx, vy])
    rs = np.random.RandomState(0)
    for _ in range(200):
        x, y = rs.uniform(-2, 3, 2)
        vx, vy = rs.uniform(-1, 1, 2)
        want = bool(should_vanish(S(x, y, vx, vy)))
        got = evaluate(code, [dict(x=x, y=y, x_vel=vx, y_vel=vy)])
        assert bool(got) == want
    mod, vec = sy.trace_modifier(lambda s: setattr(s, 'position', np.remainder(s.position, 1)))
    assert set(mod) == {'x', 'y'} and mod['x'].op == 'rem' and not vec
    node = sy.trace_value(lambda s: 1 if s.metadata['k'] else -1, 1)   # per-slot constants of the config (match_to_sample.py:171)
    assert node.op == 'select' and node.args[0].op == 'meta' and node.args[0].args == (0, 'k')
    with pytest.raises(sy.Unsupported):
        sy.trace_value(lambda s: s.path, 1)


def test_chain_generators_is_a_sequence_of_ops():
    """chain_generators (sprite_generators.py:110-128): the chained generators stay separate
    generation ops in call order."""
    import collections
    from moog import action_spaces, observers, physics as physics_lib, tasks
    from moog.state_initialization import distributions as distribs, sprite_generators as sg
    fa = distribs.Product([distribs.Continuous('x', 0., 1.)], y=0.2, shape='square', scale=0.05)
    fb = distribs.Product([distribs.Continuous('y', 0., 1.)], x=0.8, shape='circle', scale=0.05)
    gen = sg.chain_generators(sg.generate_sprites(fa, num_sprites=2), sg.generate_sprites(fb, num_sprites=3))
    c = _compiler.compile_config(
        state_initializer=lambda: collections.OrderedDict([('things', gen())]),
        physics=physics_lib.Physics(), task=tasks.CompositeTask(timeout_steps=5),
        action_space=action_spaces.Joystick(scaling_factor=0.01, action_layers='things'),
        observers={'image': observers.PILRenderer(image_size=(64, 64))})
    P = c.program
    assert P.n_ops == 2 and (P.ops[0].slot0, P.ops[0].count_max) == (0, 2)
    assert (P.ops[1].slot0, P.ops[1].count_max) == (2, 3)
    c3 = helpers.compiled('sampler_zoo_l3')      # sample_generator: a choice op, then both alternatives on the same slots
    ops = [c3.program.ops[i] for i in range(c3.program.n_ops)]
    choices = [o for o in ops if o.cell_sel == _abi.MOOG_CELL_CHOICE]
    assert [o.count_max for o in choices] == [2, 2] and choices[0].factors[0].cand_off >= 0 and choices[1].factors[0].cand_off < 0
    alts = [o for o in ops if o.cond_hdraw == 1 + choices[0].cell_arg]
    assert [o.cond_value for o in alts] == [0, 1] and alts[0].slot0 == alts[1].slot0 and alts[0].count_max == 2
    c2 = helpers.compiled('sampler_zoo_l2')      # shuffle(chain_generators(...)): a permutation op behind the generators
    ops = [c2.program.ops[i] for i in range(c2.program.n_ops)]
    shuffles = [o for o in ops if o.cell_sel == _abi.MOOG_CELL_SHUFFLE]
    assert len(shuffles) == 1 and shuffles[0].cell_arg == 4
    s0 = shuffles[0].slot0
    assert len({c2.program.slot_vcap[s] for s in range(s0, s0 + 5)}) == 1   # the four sprites and the spare slot


def test_host_randomness_in_initializer():
    """A state_initializer that draws from np.random directly (parallelogram_catch.py:36-38,64-65) must not be
    sampled once at build time and frozen into every episode: uniform / binomial draws become per-reset draws on the
    device (an op per draw, factors as expressions of them); generators the lowering has no device form for are refused."""
    import collections
    from moog import action_spaces, observers, physics as physics_lib, sprite, tasks

    def config(draw):
        def state_initializer():
            return collections.OrderedDict([('agent', [sprite.Sprite(x=draw(), y=0.5, scale=0.1)])])
        return dict(state_initializer=state_initializer, physics=physics_lib.Physics(),
                    task=tasks.CompositeTask(timeout_steps=5),
                    action_space=action_spaces.Joystick(scaling_factor=0.01, action_layers='agent'),
                    observers={'image': observers.PILRenderer(image_size=(64, 64))})
    c = _compiler.compile_config(**config(lambda: 0.5 * np.random.uniform(0.2, 0.8)))
    P = c.program
    assert P.n_hdraws == 1 and c.layout.o_hdraw >= 0
    ops = [P.ops[i] for i in range(P.n_ops)]
    assert [o.cell_sel for o in ops] == [_abi.MOOG_CELL_HDRAW, _abi.MOOG_CELL_NONE]
    assert ops[1].factors[_abi.MOOG_FAC_X].kind == _abi.MOOG_DIST_EXPR
    code = [P.dcode[ops[1].factors[_abi.MOOG_FAC_X].cand_off + k].op for k in range(8)]
    assert _abi.MOOG_X_HDRAW in code and code[-1] == _abi.MOOG_X_END   # 0.5 * (0.2 + 0.6 * u)
    with pytest.raises(NotImplementedError):
        _compiler.compile_config(**config(lambda: np.random.normal(0.5, 0.1)))
    assert 0.0 <= np.random.uniform(0., 1.) < 1.0   # the generator is restored afterwards


def test_raster_sort_key_and_network():
    """Host-side checks of two devices the HIP rasteriser relies on (csrc/moog_raster.hip):
    the 16-bit crossing key ROUND_UP(x) + ROUND_DOWN(x) is monotone in x and gives both roundings
    back, and the Batcher compare-exchange schedule sorts (0-1 principle)."""
    f = np.float32

    def round_up(x):    # Draw.c ROUND_UP, float arithmetic
        return int(np.copysign(np.floor(np.abs(x) + f(0.5)), x))

    def round_down(x):  # Draw.c ROUND_DOWN
        return int(np.copysign(np.ceil(np.abs(x) - f(0.5)), x))

    def key_up(s):
        return (s + 1) >> 1 if s >= 0 else s >> 1

    def key_down(s):
        return s >> 1 if s >= 0 else (s + 1) >> 1

    xs = []
    for n in range(-40, 41):
        for d in (-0.5, -0.25, 0.0, 0.25, 0.5):
            c = f(n + d)
            xs += [np.nextafter(c, f(-1e9)), c, np.nextafter(c, f(1e9))]
    xs = np.array(sorted(set(float(v) for v in xs)), dtype=np.float32)
    prev = None
    for x in xs:
        up, dn = round_up(x), round_down(x)
        s = up + dn
        assert key_up(s) == up and key_down(s) == dn, (x, up, dn)
        assert prev is None or s >= prev, x
        prev = s

    def network(n):
        ces, p = [], 1
        while p < n:
            q = p
            while q >= 1:
                for j in range(q % p, n - q, 2 * q):
                    for i in range(q):
                        if i + j + q <= n - 1 and (i + j) // (2 * p) == (i + j + q) // (2 * p):
                            ces.append((i + j, i + j + q))
                q //= 2
            p *= 2
        return ces

    for n in (8, 16):
        ces = network(n)
        v = (np.arange(1 << n)[:, None] >> np.arange(n)) & 1      # every 0-1 input
        for a, b in ces:
            lo, hi = np.minimum(v[:, a], v[:, b]), np.maximum(v[:, a], v[:, b])
            v[:, a], v[:, b] = lo, hi
        assert (np.diff(v, axis=1) >= 0).all(), n


def test_traced_initializer_arithmetic_matches_numpy():
    """The numpy arithmetic a state_initializer does on its own np.random draws (parallelogram_catch.py:34-68) is
    carried as expression trees (moog/_symbolic.py Sym / SymVec / SymMat).  Evaluating the trees on given uniforms must
    give exactly what numpy gives when np.random.uniform returns `low + (high - low) * u` for the same uniforms."""
    from moog import _symbolic as sy, _trace
    from moog_demos.example_configs import parallelogram_catch as pc

    def build():
        corners = pc.random_parallelogram(min_axis_ratio=0.5)
        shape = 0.075 * corners
        centres = 0.4 * corners
        centres += np.array([0.5, 0.5]) - centres[0]
        return shape, centres
    with _trace.tracing() as tr:
        sym_shape, sym_centres = build()
    assert tr.n_hdraws == 2 and isinstance(sym_shape, sy.SymMat) and sym_centres.shape == (4, 2)

    class Leaves(object):
        def __init__(self, u):
            self.u = u

        def get(self, key, boolean):
            assert key[0] == 'hdraw'
            return self.u[key[1]]
    rs = np.random.RandomState(3)
    real_uniform = np.random.uniform
    for _ in range(20):
        u = rs.uniform(size=2)
        tape = list(u)
        np.random.uniform = lambda low=0.0, high=1.0, size=None: low + (high - low) * tape.pop(0)
        try:
            ref_shape, ref_centres = build()
        finally:
            np.random.uniform = real_uniform
        for sym, ref in ((sym_shape, ref_shape), (sym_centres, ref_centres)):
            got = np.array([[sy._evaluate(c.node, Leaves(u)) for c in row] for row in sym.rows])
            # (np.sin / np.cos of an array may differ from the scalar routines in the last bit)
            assert np.max(np.abs(got - ref)) <= 1e-15, (got, ref)


def test_what_is_not_lowered_says_why():
    """Every one of the reference's 14 example configs lowers (test_reference_configs_load_unchanged); what the lowering
    does not cover is refused at construction with the reason -- no silent freezing of host randomness, no Python
    fallback: a draw numpy's generator would take once at build time, a branch on a drawn value that is no rejection
    loop, physics stepped in an initializer outside a look-ahead loop with an exit test."""
    from moog import _trace, _symbolic as sy, physics as physics_lib, sprite
    with pytest.raises(NotImplementedError) as info:
        with _trace.tracing():
            np.random.normal()
    assert 'np.random.normal' in str(info.value)
    with pytest.raises(sy.Unsupported):
        with _trace.tracing():
            _ = 1. if np.random.uniform() < 0.5 else 2.
    phys = physics_lib.Physics(updates_per_env_step=1)
    with pytest.raises(sy.Unsupported) as info:
        with _trace.tracing():
            phys.step({'a': [sprite.Sprite(x=0.5, y=0.5)]})
    assert 'look-ahead' in str(info.value)


def test_rejection_loops_over_draws_are_the_only_branches_on_draws():
    """`while not ok: a = np.random.uniform(..); ok = test(a)` in a state_initializer (match_to_sample.py:33-43) becomes
    a redraw loop on the device: the tracer answers the first test with False, must be handed the same test on a fresh
    draw, and records it as the draw's accept condition.  Any other branch on a drawn value is refused; np.sort of
    drawn values becomes compare-exchange cells."""
    from moog import _trace, _symbolic as sy

    def spread(n, gap):
        picked = [0.]
        while len(picked) < n:
            a = np.random.uniform(gap, 6. - gap)
            if all([np.abs(a - b) > gap for b in picked]):
                picked.append(a)
        return np.sort(picked)
    with _trace.tracing() as tr:
        out = spread(3, 0.5)
    draws = [op for op in tr.ops if isinstance(op, _trace.HDrawOp)]
    lets = [op for op in tr.ops if isinstance(op, _trace.HExprOp)]
    assert [len(op.accept) for op in draws] == [1, 2] and len(out) == 3
    assert len(lets) == 6 and all(v.node.op == 'hdraw' for v in out)   # three compare-exchange steps, two cells each
    # a two-way branch on a draw is not a rejection loop
    def coin():
        return 1. if np.random.uniform() < 0.5 else 2.
    with pytest.raises(sy.Unsupported):
        with _trace.tracing():
            coin()
    # neither is a loop that takes two draws per try
    def pair():
        while True:
            a, b = np.random.uniform(), np.random.uniform()
            if a + b < 1.:
                return a
    with pytest.raises(sy.Unsupported):
        with _trace.tracing():
            pair()


def test_a_generator_called_twice_is_not_a_restart():
    """`return state_initializer()` (red_green.py:155,203) is recognised by the initializer's own code appearing twice
    on the stack, not by a generator being called again: two batches from one generator stay two ops."""
    import collections
    from moog.state_initialization import distributions as distribs, sprite_generators
    gen = sprite_generators.generate_sprites(
        distribs.Product([distribs.Continuous('x', 0.1, 0.9), distribs.Continuous('y', 0.1, 0.9)], shape='square', scale=0.1),
        num_sprites=2, fail_gracefully=True)

    def init():
        first = gen()
        second = gen(without_overlapping=first)
        return collections.OrderedDict([('a', first), ('b', second)])
    tr, state = _compiler._trace_initializer(init)
    assert len(tr.ops) == 2 and [len(v) for v in state.values()] == [2, 2]
    assert not any(getattr(op, 'restart_if_short', False) for op in tr.ops)

    def init_again():
        got = gen()
        if len(got) < 2:
            return init_again()
        return collections.OrderedDict([('a', got)])
    tr, state = _compiler._trace_initializer(init_again)
    assert len(tr.ops) == 1 and tr.ops[0].restart_if_short


REFERENCE_EXPORTS = {   # the `from .x import Y` lists of the reference's five component packages (moog/*/__init__.py)
    'game_rules': ['AbstractRule', 'ChangeLayer', 'ConditionalRule', 'get_contact_counter', 'get_contact_indices',
                   'ModifyOnContact', 'CreateSprites', 'Fixation', 'ModifyMetaState', 'UpdateMetaStateValue', 'ModifySprites',
                   'Portal', 'KeepNearCenter', 'Phase', 'PhaseSequence', 'DelayedRule', 'TemporaryRule', 'TimedRule', 'Vanish',
                   'VanishByFilter', 'VanishOnContact'],
    'physics': ['AbstractForce', 'AbstractNewtonianForce', 'AbstractPhysics', 'Collision', 'ConstantSpeed', 'DistanceForce',
                'linear_force_fn', 'spring_force_fn', 'Drag', 'KineticFriction', 'DownGravity', 'Gravity',
                'DeterministicMazeWalk', 'RandomMazeWalk', 'MazePhysics', 'Physics', 'RandomForce', 'Tether',
                'TetherZippedLayers'],
    'observers': ['AbstractObserver', 'PILRenderer', 'RawState', 'polygon_modifiers'],
    'action_spaces': ['AbstractActionSpace', 'Composite', 'Grid', 'Joystick', 'SetPosition'],
    'tasks': ['AbstractTask', 'CompositeTask', 'ContactReward', 'Reset', 'StayAlive'],
    'env_wrappers': ['AbstractEnvironmentWrapper', 'LoggingEnvironment', 'MultiAgentEnvironment', 'SimulationEnvironment'],
    'maze_lib': ['Maze', 'generate_random_maze_matrix', 'get_connected_open_blob'],
}


def test_reference_import_surface():
    """Every name the reference's packages export exists under the same name, and so do the module paths its own tests
    and configs import (tests/moog/**: `from moog.physics import collisions`, `from moog.observers import pil_renderer`,
    `from moog.env_wrappers import simulation / gym_wrapper`, `moog.game_rules.vanish.Vanish`, the sprite module's
    functions).  When /root/reference is there the lists are read from its __init__ files instead of the table above."""
    import importlib
    import re
    exports = {k: list(v) for k, v in REFERENCE_EXPORTS.items()}
    ref = '/root/reference/moog'
    if os.path.isdir(ref):
        for pkg in exports:
            with open(os.path.join(ref, pkg, '__init__.py')) as f:
                found = re.findall(r'^from \.\S* import (\w+)', f.read(), flags=re.M)
            assert sorted(found) == sorted(exports[pkg]), pkg
    for pkg, names in exports.items():
        m = importlib.import_module('moog.' + pkg)
        for n in names:
            assert hasattr(m, n), 'moog.%s.%s' % (pkg, n)
    for path, attr in (('moog.physics.collisions', 'Collision'), ('moog.observers.pil_renderer', 'PILRenderer'),
                       ('moog.observers.polygon_modifiers', 'TorusGeometry'), ('moog.observers.color_maps', 'hsv_to_rgb'),
                       ('moog.env_wrappers.simulation', 'SimulationEnvironment'), ('moog.env_wrappers.gym_wrapper', 'GymWrapper'),
                       ('moog.game_rules.vanish', 'Vanish'), ('moog.game_rules.contact_rules', 'get_contact_indices'),
                       ('moog.game_rules.modify_meta_state', 'UpdateMetaStateValue'), ('moog.game_rules.timing', 'TimedRule'),
                       ('moog.physics.tether_physics', 'Tether'), ('moog.tasks.contact_reward', 'ContactReward'),
                       ('moog.action_spaces.joystick', 'Joystick'), ('moog.observers.abstract_observer', 'AbstractObserver'),
                       ('moog.state_initialization.distributions', 'Continuous'),
                       ('moog.state_initialization.sprite_generators', 'generate_sprites'),
                       ('moog.sprite', 'update_sprite'), ('moog.sprite', 'segment_crossing_coefficients'),
                       ('moog.sprite', 'segment_crossings'), ('moog.sprite', 'sprite_edge_crossings'), ('moog.shapes', 'border_walls')):
        assert hasattr(importlib.import_module(path), attr), '%s.%s' % (path, attr)
    from moog.physics import collisions   # noqa: F401  (the statement itself, as tests/moog/physics/test_collisions.py:28 has it)
    from moog import game_rules
    assert game_rules.vanish.Vanish is game_rules.Vanish


def test_segment_helpers_and_update_sprite():
    """The sprite module's functions (sprite.py:51-224), host numpy: crossing coefficients of two segment sets with the
    reference's 1e-8 in the denominator; update_sprite replaces factors of a recipe."""
    from moog import sprite
    s0, e0 = np.array([[0., 0.], [0., 1.]]), np.array([[1., 1.], [1., 1.]])
    s1, e1 = np.array([[0., 1.], [5., 5.]]), np.array([[1., 0.], [6., 5.]])
    A, B = sprite.segment_crossing_coefficients(s0, e0, s1, e1)
    assert A.shape == (2, 2) and abs(A[0, 0] - 0.5) < 1e-7 and abs(B[0, 0] - 0.5) < 1e-7
    pts, inds = sprite.segment_crossings(s0, e0, s1, e1)
    assert inds.tolist() == [[0, 0]] and np.allclose(pts, [[0.5, 0.5]], atol=1e-7)

    class Live(object):   # what the reference passes: anything with a closed path
        def __init__(self, v):
            self.path = type('P', (), {'vertices': np.concatenate([v, v[:1]])})
    sq = np.array([[0., 0.], [1., 0.], [1., 1.], [0., 1.]])
    pts, inds = sprite.sprite_edge_crossings(Live(sq), Live(sq + 0.5))
    assert sorted(map(tuple, np.round(pts, 6).tolist())) == [(0.5, 1.0), (1.0, 0.5)]
    sp = sprite.Sprite(x=0.2, y=0.3, c0=10)
    sprite.update_sprite(sp, x=0.7, c0=99, shape='triangle')
    assert sp.factors['x'] == 0.7 and sp.factors['c0'] == 99 and sp.factors['shape'] == 'triangle'
    with pytest.raises(TypeError):
        sprite.update_sprite(sp, colour=1)


def test_config_local_vanish_and_meta_state_value():
    """A config that subclasses game_rules.Vanish (vanish.py:9-39) with the reference's own pattern -- the indices of the
    layer's sprites that pass a test -- lowers to the device's filtered vanish; index functions that are not a per-sprite
    filter are refused with the reason.  UpdateMetaStateValue (modify_meta_state.py:28-48) is a host-side rule."""
    import collections
    from moog import action_spaces, game_rules, observers, physics as physics_lib, sprite, tasks

    class VanishLeft(game_rules.Vanish):
        def _get_vanish_inds(self, state):
            return [i for i, s in enumerate(state[self._layer]) if s.x < 0.25]

    class VanishFirstTwo(game_rules.Vanish):
        def _get_vanish_inds(self, state):
            return [i for i, _ in enumerate(state[self._layer])][:1]

    def config(rule):
        return dict(
            state_initializer=lambda: collections.OrderedDict(
                [('prey', [sprite.Sprite(x=0.1 + 0.2 * k, y=0.5, scale=0.05, c0=128) for k in range(4)]),
                 ('agent', [sprite.Sprite(x=0.5, y=0.2, scale=0.1)])]),
            physics=physics_lib.Physics(), task=tasks.ContactReward(1., 'agent', 'prey'),
            action_space=action_spaces.Grid(0.1, action_layers='agent', control_velocity=True),
            observers={'image': observers.PILRenderer(image_size=(64, 64))},
            game_rules=(rule, game_rules.UpdateMetaStateValue('phase', 'go')), meta_state_initializer=lambda: {'phase': ''})

    c = _compiler.compile_config(**config(VanishLeft('prey')))
    P = c.program
    assert P.n_rules == 1 and P.rules[0].kind == _abi.MOOG_RULE_VANISH_BY_FILTER and P.rules[0].filter == _abi.MOOG_FILTER_EXPR
    m = {'phase': ''}
    game_rules.UpdateMetaStateValue('phase', 'go').step(None, m)
    assert m == {'phase': 'go'}
    with pytest.raises(NotImplementedError):
        _compiler.compile_config(**config(VanishFirstTwo('prey')))


def test_rule_interval_probe_sees_every_draw():
    """A callable interval of a TimedRule family rule is redrawn at every reset by the reference (timing.py:47): it is
    lowered when its randomness is ONE np.random.randint draw, kept when it is a constant, and refused when it draws any
    other way (np.random.uniform / choice, the `random` module, a randint imported by name) -- never frozen at the value
    of the probe call.  The host's generators are left untouched by the probe."""
    import random as py_random
    from numpy.random import randint as captured
    from moog import game_rules as gr
    np.random.seed(3)
    py_random.seed(3)
    before = (np.random.get_state()[1].copy(), py_random.getstate())
    assert gr.DelayedRule(lambda: np.random.randint(10, 100), [])._random == (1, 10.0, np.inf, 100.0)
    assert gr.TemporaryRule(lambda: np.random.randint(5, 9), [])._random == (2, 0.0, 5.0, 9.0)
    assert gr.DelayedRule(lambda: 7, [])._step_interval == (7.0, np.inf)
    # two draws: a random start, then a random duration (timing.py:84-86); other two-draw forms stay refused
    assert gr.DelayedRule(lambda: np.random.randint(3, 9), [], duration=lambda: np.random.randint(2, 7))._random == (3, 3.0, 2.0, 9.0, 7)
    with pytest.raises(NotImplementedError):
        gr.TimedRule(lambda: (np.random.randint(0, 4), np.random.randint(10, 20)), [])   # (the stop is not start + a draw)
    for fn in (lambda: int(np.random.uniform(10, 100)), lambda: np.random.choice([3, 5]), lambda: py_random.randint(1, 5),
               lambda: captured(10, 100), lambda: np.random.randint(0, 3) + np.random.randint(0, 3)):
        with pytest.raises(NotImplementedError):
            gr.DelayedRule(fn, [])
    assert np.array_equal(before[0], np.random.get_state()[1]) and before[1] == py_random.getstate()


def test_program_step_kernel_and_spec_source():
    """moog_program_step_kernel needs no device: variant, register-allocation variant and the FNV-1a hash the specialised
    kernel's file name carries (computed here in Python as a check); the generated include reproduces the program's doubles
    exactly (hexadecimal literals)."""
    from moog import _spec
    for name, variant in (('colliding_predators_32', 0), ('cleanup', 1), ('pacman', 2)):
        P = helpers.compiled(name).program
        v, w, h = _spec.kernel_of(P)
        assert v == variant and w in (2, 3, 4), (name, v, w)
        raw = bytes(P)
        assert len(raw) == ctypes.sizeof(_abi.Program)
        fnv = 1469598103934665603
        for b in raw[::1]:
            fnv = ((fnv ^ b) * 1099511628211) & 0xffffffffffffffff
        assert fnv == h, name
        assert os.path.basename(_spec.path_of(P)) == 'step_%016x_d%dw%d.so' % (h, v, w)
    src = _spec.source_of(helpers.compiled('colliding_predators_32').program)
    assert 'MOOG_SPEC_HASH' in src and 'static const moog_program_t MOOG_SPEC_PROGRAM = {' in src
    assert float.fromhex(float.hex(0.1)) == 0.1 and '0x1.' in src
