"""Environment (reference: moog/environment.py:28-158), batched on one MI355X.

`BatchedEnvironment(**config, num_envs=N)` keeps the reference's method names
(`reset`, `step`, `observation`, `observation_spec`, `action_spec`,
`state`-like accessors) with a leading env axis: step_type int32[N], reward
float64[N] (NaN where the reference returns None), discount float64[N],
observation {'image': uint8[N,H,W,3]} -- all torch tensors on the device; a config with several
PILRenderers gets one such tensor per renderer key (the engine's extra views), one with none only
its RawState entries; a SpriteTable observer's entry is its float32 / float16 tensor [N, rows, columns], rewritten in place
like the frames, a Segmentation observer's its uint8 id image [N, H, W], drawn with the frames, a RaySensor observer's its
float32 / float16 readings [N, rays, 2], kept beside the tables' tensors and rewritten with them, a Contacts observer's its
uint8 overlap flags [N, R0, R1] or [N, R0, layers], kept and rewritten likewise.
Auto-reset follows environment.py:100-101 per env: the call after a LAST
timestep ignores that env's action and returns a FIRST timestep.

`Environment(**config)` is the single-env facade with numpy/scalar outputs.
"""
import collections
import ctypes

import numpy as np

from . import _abi
from . import _compiler
from . import _dm_env as dm_env
from . import _engine
from .observers import contacts as contacts_lib, ray_sensor, segmentation, sprite_table

# How an observer goes from a lowered config to the engine, kind by kind, in the order they are attached.  field: Compiled's
# [(key, descriptor)]; add / bind: the engine's functions that take the descriptor and the tensor; tensors: the env's dict
# that holds the tensor under the observer's key; index: the env's dict {key: engine index}; observe: the engine's function
# that refreshes every bound observer of the kind, None for the kinds drawn with the frames; spec: descriptor -> specs.Array
# of one env's observation.
ObserverKind = collections.namedtuple('ObserverKind', ['field', 'add', 'bind', 'tensors', 'index', 'observe', 'spec'])
OBSERVER_KINDS = (
    ObserverKind('views', 'moog_engine_add_view', 'moog_engine_set_view_image', 'view_images', '_view_index', None,
                 lambda R: dm_env.specs.Array(shape=(int(R.height), int(R.width), 3), dtype=np.uint8)),
    ObserverKind('tables', 'moog_engine_add_table', 'moog_engine_set_table_buffer', 'tables', '_table_index',
                 'moog_engine_observe_tables', sprite_table.table_spec),
    ObserverKind('sensors', 'moog_engine_add_sensor', 'moog_engine_set_sensor_buffer', 'tables', '_sensor_index',
                 'moog_engine_observe_sensors', ray_sensor.sensor_spec),
    ObserverKind('contacts', 'moog_engine_add_contacts', 'moog_engine_set_contacts_buffer', 'tables', '_contacts_index',
                 'moog_engine_observe_contacts', contacts_lib.contacts_spec),
    ObserverKind('segmentations', 'moog_engine_add_segmentation', 'moog_engine_set_segmentation_image', 'view_images',
                 '_segmentation_index', None, segmentation.segmentation_spec),
)
# The tensors a SubBatchedEnvironment hands a part: slices of its own.
PartBuffers = collections.namedtuple('PartBuffers', ['state_f64', 'state_i32', 'reward', 'discount', 'step_type', 'image',
                                                     'view_images', 'repeat_count', 'tables'])

_FAULT_EXC = (
    (_abi.MOOG_FAULT_SAMPLER_EXHAUSTED, RecursionError,
     'max_recursion_depth exceeded trying to initialize a non-overlapping sprite.'),
    (_abi.MOOG_FAULT_ODD_PORTALS, ValueError, 'There must be an even number of portals.'),
    (_abi.MOOG_FAULT_BAD_NORMAL, ValueError, 'collision_normal_norm is not close to 1.'),
    (_abi.MOOG_FAULT_INJECT_UNDERRUN, RuntimeError, 'injected uniform buffer exhausted.'),
    (_abi.MOOG_FAULT_DIST_EXHAUSTED, ValueError,
     'Maximum number of tried exceeded when trying to sample from a distribution.'),
    (_abi.MOOG_FAULT_PHASE_END, IndexError, 'tuple index out of range (PhaseSequence ran past its last phase).'),
    (_abi.MOOG_FAULT_LAYER_FULL, RuntimeError,
     'a rule appended to a layer whose slot capacity is used up (raise layer_capacity).'),
    (_abi.MOOG_FAULT_TETHER_ZIP, ValueError,
     'All layers fed into TetherAcrossLayers must have the same number of sprites.'),
    (_abi.MOOG_FAULT_OFF_GRID, ValueError, 'Object is not on the maze grid.'),
)


class BatchedEnvironment(object):
    """N independent MOOG environments stepped by one HIP engine handle."""

    def __init__(self, state_initializer, physics, task, action_space, observers, game_rules=(),
                 meta_state_initializer=None, num_envs=1, device=None, seed=0, env_index0=0,
                 layer_capacity=None, keep_sprite_factors=False, reset_pool='auto', specialize=False, action_repeat=1,
                 _compiled=None, _buffers=None):
        # action_repeat: k env-steps per step() call with the call's action ("frame skip"), inside one launch of the step kernel
        # (set_action_repeat; include/moog_engine.h moog_engine_set_action_repeat).  What cannot be repeated on the device is
        # refused here, before anything touches it.
        self._auto_capacity = layer_capacity == 'auto' or (isinstance(layer_capacity, dict) and bool(layer_capacity.get('auto')))
        self._host_rules = [r for r in game_rules if getattr(r, 'host_side', False)]
        self._meta_state_initializer = meta_state_initializer
        self._action_repeat = self._check_action_repeat(action_repeat)
        import torch
        self._torch = torch
        self._lib = _engine.load_library()  # raises when the HIP extension is missing
        # specialize: True compiles (once; needs hipcc, not a GPU; ~20 s) a step kernel for this very program -- same source, the
        # program a compile-time constant, bit-identical results, faster (moog/_spec.py).  Whatever the argument, an engine uses
        # such a kernel when one has been built for its program (moog_engine_step_kernel; MOOG_STEP_SPEC=0 turns that off).
        self._specialize = bool(specialize)
        # reset_pool: build every env's NEXT episode beside the step kernels and take it over when the episode ends
        # (moog_engine_set_reset_pool; same results, bit for bit).  'auto': on for configs whose state_initializer plays
        # physics forward (bounce_box_contact_prediction, red_green: a reset there costs as much as a hundred steps of the
        # whole batch) when the engine can (see self.reset_pool); True: on, or EngineError; False: off.
        self._reset_pool_arg = reset_pool
        if not torch.cuda.is_available():
            raise _engine.EngineError('no HIP device available: the MOOG engine has no CPU path')
        # (_compiled / _buffers: a SubBatchedEnvironment builds its parts over one lowered program and slices of one set of
        #  tensors)
        # layer_capacity: {layer: slots} for the layers rules append to (the reference's lists are unbounded,
        # create_sprites.py:34, change_layer.py:43; the engine's are slots), None for the default (initial count + 8), or
        # 'auto' / {'auto': True, layer: initial slots, ...}: start from those capacities and GROW -- whenever a step leaves
        # a layer's high-water mark (moog_engine_layer_usage) within a quarter of its capacity, the engine is re-created with
        # that layer doubled and every env's records are moved to the new layout before the next call (_grow_layers).
        # 'auto' also FITS, once: after `fit_after` calls of step() (default 128; {'auto': True, 'fit_after': k}; 0: never) the
        # layers are sized to what the batch has needed so far, high-water x 1.25 (fit_layer_capacity): a record holds every slot's
        # vertices, so roomy initial capacities cost envs per CU for the whole run otherwise (first_person_predators_prey at
        # {prey: 32, predators: 96}: one env per CU, 0.88 M env-steps/s; fitted: two, 1.6 M).  Growth on demand goes on afterwards.
        self._fit_after, self._n_step_calls = 0, 0
        if layer_capacity == 'auto':
            self._auto_capacity, layer_capacity, self._fit_after = True, None, 128
        elif isinstance(layer_capacity, dict) and layer_capacity.get('auto'):
            self._auto_capacity = True
            self._fit_after = int(layer_capacity.get('fit_after', 128))
            layer_capacity = {k: v for k, v in layer_capacity.items() if k not in ('auto', 'fit_after')}
        self._config_args = (state_initializer, physics, task, action_space, observers, game_rules, meta_state_initializer)
        self._keep_sprite_factors = keep_sprite_factors
        self._seed, self._env_index0 = int(seed), int(env_index0)
        self.compiled = _compiled if _compiled is not None else _compiler.compile_config(
            state_initializer, physics, task, action_space, observers, game_rules,
            meta_state_initializer, layer_capacity=layer_capacity,
            keep_sprite_factors=keep_sprite_factors)
        self.physics = physics
        self.task = task
        self.action_space = action_space
        self.observers = observers
        self.game_rules = game_rules
        self.num_envs = int(num_envs)
        # meta_state (environment.py:60-63,87): a host-side Python object per environment, touched only by
        # `ModifyMetaState` rules (arbitrary Python, never sprites): one object for a batch of one, a list of
        # num_envs objects otherwise.  Those rules run in a host loop over the envs, and every step then reads the
        # auto-reset flags back (one device-to-host copy per step): convenient, not fast.
        self._meta_state = None
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None \
            else torch.device(device)
        P, L = self.compiled.program, self.compiled.layout
        self.layout = L
        n = self.num_envs
        if _buffers is not None:
            for name in PartBuffers._fields:
                setattr(self, name, getattr(_buffers, name))
        else:
            with torch.cuda.device(self.device):
                (self.state_f64, self.state_i32, self.reward, self.discount, self.step_type,
                 self.image) = self.allocate_buffers(torch, L, P, n, self.device)
            self.view_images = None
            self.repeat_count = None
            self.tables = None
        if self.repeat_count is None:
            # env-steps each env took in the last step() call: action_repeat, fewer where the episode ended inside the call,
            # 0 where the call reset the env (a FIRST timestep) and after reset()
            self.repeat_count = torch.zeros((n,), dtype=torch.int32, device=self.device)
        if self.view_images is None:
            with torch.cuda.device(self.device):
                self.view_images = self.allocate_view_buffers(torch, self.compiled, n, self.device)
        if self.tables is None:
            with torch.cuda.device(self.device):
                self.tables = self.allocate_table_buffers(torch, self.compiled, n, self.device)
        # frames per PILRenderer key, in the config's order: the primary's `image` and the extra views' tensors
        self._frames = {}
        if self.compiled.observer_key is not None:
            self._frames[self.compiled.observer_key] = self.image
        self._frames.update(self.view_images)
        if self._specialize:
            from . import _spec
            _spec.build(P)
        self._open_engine()
        self._out = _abi.StepOut()
        self._out.reward = ctypes.cast(self.reward.data_ptr(), ctypes.POINTER(ctypes.c_double))
        self._out.discount = ctypes.cast(self.discount.data_ptr(), ctypes.POINTER(ctypes.c_double))
        self._out.step_type = ctypes.cast(self.step_type.data_ptr(), ctypes.POINTER(ctypes.c_int32))
        if self.compiled.observer_key is not None:   # (no PILRenderer: the program draws no frames, the calls pass none)
            self._out.image = ctypes.cast(self.image.data_ptr(), ctypes.POINTER(ctypes.c_uint8))
        self._composite = hasattr(action_space, 'action_spaces')
        self._n_actions = max(1, int(P.n_actions))
        self._is_grid = (not self._composite) and P.action.kind == _abi.MOOG_ACTION_GRID
        self._dynamic_layers = any(P.layer_dynamic[i] for i in range(P.n_layers))
        # Device-side faults (the reference's exceptions): True = deferred -- the kernels OR fault bits
        # into a host-visible word that every call polls first, so a fault raises at the latest in the
        # call after the one that caused it, without a per-step synchronisation; 'sync' = also
        # synchronise and check after every call (the exception comes from the call itself);
        # False = never check.  Runs with injected uniforms / run-time sprite creation check at once.
        self.check_faults = True
        self._cost = self._perm = None
        self._action_f32 = False
        self._apply_action_repeat()
        self._apply_reset_pool()
        self._setup_color_fn()

    def _check_action_repeat(self, k):
        """k as an int, or the reason an engine like this one cannot repeat an action on the device."""
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= _abi.MOOG_MAX_ACTION_REPEAT:
            raise ValueError('action_repeat must be an integer in 1 .. %d, got %r' % (_abi.MOOG_MAX_ACTION_REPEAT, k))
        k = int(k)
        if k == 1:
            return k
        if self._host_rules or self._meta_state_initializer is not None:
            raise NotImplementedError(
                'action_repeat=%d: host-side meta-state rules (ModifyMetaState / a meta_state_initializer) run in Python once per '
                'step() call, the repeated env-steps run inside one kernel launch: the rules would miss %d of every %d env-steps '
                '(call step() %d times instead)' % (k, k - 1, k, k))
        if self._auto_capacity:
            raise NotImplementedError(
                "action_repeat=%d: layer_capacity='auto' grows a layer between calls, when its high-water mark comes within a "
                "margin sized for ONE env-step of appends; %d env-steps per call can overflow it before the host looks "
                "(pass layer_capacity={layer: slots}; env.layer_usage() reports the demand)" % (k, k))
        return k

    def _apply_action_repeat(self):
        _engine.check(self._lib, self._lib.moog_engine_set_action_repeat(
            self._handle, self._action_repeat, ctypes.c_void_p(self.repeat_count.data_ptr())))

    @property
    def action_repeat(self):
        return self._action_repeat

    def set_action_repeat(self, k):
        """k env-steps per step() call from the next call on (1: the reference's one step per call).  Every env holds the
        call's action for up to k env-steps inside one launch of the step kernel and stops at the first one that ends its
        episode; the timestep carries the rewards' sum (float64, in step order), the last step's step_type / discount and the
        frame after it; `repeat_count` says how many env-steps each env took.  The state after the call is, bit for bit, the
        state after that many single calls."""
        self._action_repeat = self._check_action_repeat(k)
        self._apply_action_repeat()

    def _open_engine(self):
        """A new engine handle over `self.compiled` and the records as they are: create, load_state, and the config's
        observers attached (the constructor; _grow_layers, over the new program and the moved records)."""
        torch = self._torch
        self._handle = ctypes.c_void_p()
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        with torch.cuda.device(self.device):   # (the engine calls hipSetDevice: keep torch's current device)
            _engine.check(self._lib, self._lib.moog_engine_create(
                ctypes.byref(self.compiled.program), self.num_envs, dev_index, self._seed, self._env_index0,
                ctypes.byref(self._handle)))
        view = _abi.StateView()
        view.f64 = ctypes.cast(self.state_f64.data_ptr(), ctypes.POINTER(ctypes.c_double))
        view.i32 = ctypes.cast(self.state_i32.data_ptr(), ctypes.POINTER(ctypes.c_int32))
        _engine.check(self._lib, self._lib.moog_engine_load_state(self._handle, ctypes.byref(view)))
        self._attach_observers()

    def _attach_observers(self):
        """Every observer of OBSERVER_KINDS in the config: described to the engine (its add function), bound to its own tensor
        (its bind function), and its engine index kept under its key.  An extra view and a segmentation are drawn whenever
        the primary's frames are; a sprite table, a ray sensor and a contacts observer are written by every reset / step call
        and by observation()."""
        for kind in OBSERVER_KINDS:
            index = {}
            for key, desc in getattr(self.compiled, kind.field):
                idx = ctypes.c_int32()
                with self._torch.cuda.device(self.device):
                    _engine.check(self._lib, getattr(self._lib, kind.add)(self._handle, ctypes.byref(desc), ctypes.byref(idx)))
                _engine.check(self._lib, getattr(self._lib, kind.bind)(
                    self._handle, idx.value, ctypes.c_void_p(getattr(self, kind.tensors)[key].data_ptr())))
                index[key] = idx.value
            setattr(self, kind.index, index)

    def segmentation_rows(self, key):
        """[(layer name, index in layer)] for every row of the Segmentation observer `key`: value v of an 'instance' mask is
        row v - 1 (the rows of a SpriteTable over the same layers); value v of a 'layer' mask is the v-th chosen layer."""
        return list(self.compiled.segmentation_rows[key])

    def contact_rows(self, key):
        """(rows_0, rows_1) of the Contacts observer `key`: [(layer name, index in layer)] for every row of each argument --
        the rows of a SpriteTable over the same layers.  In 'layer' mode column l is the l-th layer of `layers_1`."""
        rows_0, rows_1 = self.compiled.contact_rows[key]
        return list(rows_0), list(rows_1)

    def ray_rows(self, key):
        """[(layer name, index in layer)] for every row of the RaySensor observer `key`: id v of an 'instance' sensor is row
        v - 1 (the rows of a SpriteTable over the same layers); id v of a 'layer' sensor is the v-th chosen layer; 0 is no
        hit."""
        return list(self.compiled.sensor_rows[key])

    def ray_directions(self, key):
        """The [num_rays, 2] float64 unit vectors the engine was given for the RaySensor observer `key`."""
        T = dict(self.compiled.sensors)[key]
        return np.array([[T.dirs[k][0], T.dirs[k][1]] for k in range(int(T.n_rays))], dtype=np.float64)

    def _observe_tables(self):
        for kind in OBSERVER_KINDS:
            if kind.observe and getattr(self.compiled, kind.field):
                with self._torch.cuda.device(self.device):
                    _engine.check(self._lib, getattr(self._lib, kind.observe)(self._handle, self._stream()))

    @staticmethod
    def _allocate_observer_buffers(torch, compiled, n, device, tensors):
        """{key: zeros [n] + the observer's spec} for the observers of the kinds kept in the dict `tensors`, kind after kind."""
        bufs = {}
        for kind in OBSERVER_KINDS:
            if kind.tensors == tensors:
                for key, desc in getattr(compiled, kind.field):
                    spec = kind.spec(desc)
                    bufs[key] = torch.zeros((n,) + tuple(spec.shape), dtype=getattr(torch, spec.dtype.name), device=device)
        return bufs

    @staticmethod
    def allocate_table_buffers(torch, compiled, n, device):
        """{key: float32 / float16 [n, rows, columns]} for the config's SpriteTables and {key: float32 / float16
        [n, rays, 2]} for its RaySensors and {key: uint8 [n, R0, R1] or [n, R0, layers]} for its Contacts observers."""
        return BatchedEnvironment._allocate_observer_buffers(torch, compiled, n, device, 'tables')

    def table_rows(self, key):
        """[(layer name, index in layer)] for every row of the SpriteTable observer `key`."""
        return list(self.compiled.table_rows[key])

    def table_columns(self, key):
        """The column names of the SpriteTable observer `key`."""
        if key not in self.compiled.table_rows:
            raise KeyError('%r is not a SpriteTable observer of this config' % (key,))
        return tuple(self.observers[key].columns)

    @staticmethod
    def allocate_view_buffers(torch, compiled, n, device):
        """{key: uint8 [n, H, W, 3]} for the extra views (the config's PILRenderers after the first) and {key: uint8
        [n, H, W]} for its Segmentation observers."""
        return BatchedEnvironment._allocate_observer_buffers(torch, compiled, n, device, 'view_images')

    def _setup_color_fn(self):
        """PILRenderer(color_to_rgb=<a callable>): the callable is evaluated here, on the host, once per distinct colour
        triple; the rasteriser takes the results per (env, sprite slot) from `self._rgb` (moog_engine_set_color_override).
        The engine's calls are then split -- step without frames, colours, frames -- and one small device-to-host read per
        call asks whether any colour changed: convenient, not fast (like the host-side ModifyMetaState rules)."""
        from .observers import pil_renderer
        ren = [o for o in self.observers.values() if isinstance(o, pil_renderer.PILRenderer)]
        self._color_fn = ren[0].color_to_rgb if ren and ren[0]._cmap == 'callable' else None
        if self._color_fn is None:
            return
        torch = self._torch
        S = self.layout.S
        self._rgb = torch.zeros((self.num_envs, S), dtype=torch.int32, device=self.device)
        self._rgb_seen = None          # colour bit patterns the entries of _rgb were computed from
        self._rgb_done = torch.zeros((self.num_envs, S), dtype=torch.bool, device=self.device)
        self._rgb_cache = {}
        _engine.check(self._lib, self._lib.moog_engine_set_color_override(self._handle, ctypes.c_void_p(self._rgb.data_ptr())))
        self._out_noimg = _abi.StepOut()
        self._out_noimg.reward, self._out_noimg.discount = self._out.reward, self._out.discount
        self._out_noimg.step_type = self._out.step_type

    @staticmethod
    def _call_color_fn(fn, triple):
        """color_to_rgb on one colour triple, the way pil_renderer.py:108-110 and Pillow's ink conversion treat the result:
        three integers, clipped to 0 .. 255.  Components that hold an integral value are passed as Python ints (a Sprite
        keeps the numbers it was given; the engine's records hold float64)."""
        import numbers
        args = tuple(int(v) if float(v).is_integer() else float(v) for v in triple)
        out = list(fn(args))
        if len(out) != 3:
            raise ValueError('color_to_rgb must return three components, got %r' % (out,))
        rgb = 0
        for k, v in enumerate(out):
            if not isinstance(v, (numbers.Integral, np.integer)):
                raise TypeError('color_to_rgb returned %r: Pillow takes integer colour components' % (v,))
            rgb |= min(255, max(0, int(v))) << (8 * k)
        return rgb

    def _refresh_colors(self):
        torch = self._torch
        L, S = self.layout, self.layout.S
        col = self.state_f64[:, L.o_color:L.o_color + 3 * S].view(torch.int64).view(self.num_envs, S, 3)
        alive = (self.state_i32[:, L.o_flags:L.o_flags + S] & _abi.MOOG_F_ALIVE) != 0
        if self._rgb_seen is None:
            need = alive
        else:
            need = alive & ((col != self._rgb_seen).any(-1) | ~self._rgb_done)
        idx = need.nonzero()            # (the one synchronising read of the call)
        if idx.shape[0]:
            bits = col[idx[:, 0], idx[:, 1]].cpu().numpy()
            vals = bits.view(np.float64)
            out = np.empty(len(bits), np.int32)
            for i in range(len(bits)):
                key = bits[i].tobytes()
                rgb = self._rgb_cache.get(key)
                if rgb is None:
                    rgb = self._rgb_cache[key] = self._call_color_fn(self._color_fn, vals[i])
                out[i] = rgb
            self._rgb[idx[:, 0], idx[:, 1]] = torch.as_tensor(out, device=self.device)
            self._rgb_done[idx[:, 0], idx[:, 1]] = True
        # (a slot without a live sprite forgets what it held: the sprite that comes to life there is evaluated again even if a
        #  host-side edit gave it the colour bits the snapshot already has)
        self._rgb_done &= alive
        self._rgb_seen = col.clone()

    def _render_with_colors(self):
        self._refresh_colors()
        with self._torch.cuda.device(self.device):
            _engine.check(self._lib, self._lib.moog_engine_render(
                self._handle, ctypes.c_void_p(self.image.data_ptr()), self._stream()))

    def _apply_reset_pool(self):
        want = self._reset_pool_arg
        P = self.compiled.program
        if want == 'auto':
            want = any(P.ops[o].cell_sel == _abi.MOOG_CELL_SIMULATE for o in range(P.n_ops))
            strict = False
        else:
            strict = bool(want)
        self.reset_pool_refusal = None
        if want:
            with self._torch.cuda.device(self.device):
                rc = self._lib.moog_engine_set_reset_pool(self._handle, 1)
            if rc != 0:
                if strict:
                    _engine.check(self._lib, rc)
                self.reset_pool_refusal = self._lib.moog_last_error().decode()

    @property
    def reset_pool(self):
        """The engine's reset pool: {'on', 'fills' (fill launches), 'adopted' (episodes opened from the pool), 'in_place'
        (episodes opened by a reset inside the step kernel), 'rejected' (pool records dropped by the input check), 'waited'
        (take-overs that waited for a fill)}; synchronises.  `reset_pool_refusal` holds the engine's reason when
        reset_pool='auto' wanted the pool and could not have it."""
        on, st = ctypes.c_int32(), (ctypes.c_int64 * 5)()
        _engine.check(self._lib, self._lib.moog_engine_get_reset_pool(self._handle, ctypes.byref(on), st))
        return dict(on=bool(on.value), fills=int(st[0]), adopted=int(st[1]), in_place=int(st[2]), rejected=int(st[3]),
                    waited=int(st[4]))

    @property
    def kernel_variant(self):
        """(step-kernel variant 0 / 1 / 2, late reset) -- include/moog_engine.h moog_engine_kernel_variant."""
        v, late = ctypes.c_int32(), ctypes.c_int32()
        _engine.check(self._lib, self._lib.moog_engine_kernel_variant(self._handle, ctypes.byref(v), ctypes.byref(late)))
        return int(v.value), bool(late.value)

    @property
    def env_prefix_slots(self):
        """Leading sprite slots the rasteriser keeps in a cached picture per env (moog_engine_env_prefix); 0: unused."""
        v = ctypes.c_int32()
        _engine.check(self._lib, self._lib.moog_engine_env_prefix(self._handle, ctypes.byref(v)))
        return int(v.value)

    @staticmethod
    def allocate_buffers(torch, L, P, n, device):
        """The state records and step outputs of n envs (the engine borrows their device pointers)."""
        return (torch.zeros((n, L.f64_per_env), dtype=torch.float64, device=device),
                torch.zeros((n, L.i32_per_env), dtype=torch.int32, device=device),
                torch.full((n,), float('nan'), dtype=torch.float64, device=device),
                torch.full((n,), float('nan'), dtype=torch.float64, device=device),
                torch.zeros((n,), dtype=torch.int32, device=device),
                torch.zeros((n, P.render.height, P.render.width, 3), dtype=torch.uint8, device=device))

    def enable_cost_schedule(self, enabled=True):
        """Launch the step kernel's workgroups in order of descending per-env cost of the
        previous step (longest-processing-time first): the envs with clustered contacts
        start first instead of landing in the under-filled tail of the launch.  The engine
        re-sorts the order after every step on a side stream.  A pure scheduling hint --
        results are identical."""
        torch = self._torch
        if enabled:
            self._cost = torch.zeros((self.num_envs,), dtype=torch.float32, device=self.device)
            self._perm = torch.arange(self.num_envs, dtype=torch.int32, device=self.device)
            with torch.cuda.device(self.device):
                _engine.check(self._lib, self._lib.moog_engine_set_schedule(
                    self._handle, ctypes.c_void_p(self._perm.data_ptr()),
                    ctypes.c_void_p(self._cost.data_ptr())))
        else:
            self._cost = self._perm = None
            _engine.check(self._lib, self._lib.moog_engine_set_schedule(self._handle, None, None))

    def step_kernel(self):
        """'specialised' when the engine steps with a kernel compiled for this program (moog/_spec.py), else 'generic'."""
        v = ctypes.c_int32()
        _engine.check(self._lib, self._lib.moog_engine_step_kernel(self._handle, ctypes.byref(v)))
        return 'specialised' if v.value else 'generic'

    def raster_path(self, view_key=None):
        """Which rasteriser draws this engine's frames: 'mask' (csrc/moog_raster_mask_core.h) or 'spans'
        (csrc/moog_raster_kernel.h) -- moog_engine_raster_path.  view_key: the PILRenderer observer's key (default: the
        first renderer, the program's own frames; another key: that extra view's, moog_engine_view_raster_path)."""
        v = ctypes.c_int32()
        if view_key is None or view_key == self.compiled.observer_key:
            _engine.check(self._lib, self._lib.moog_engine_raster_path(self._handle, ctypes.byref(v)))
        else:
            if view_key not in self._view_index:
                raise KeyError('%r is not a PILRenderer observer of this config' % (view_key,))
            _engine.check(self._lib, self._lib.moog_engine_view_raster_path(self._handle, self._view_index[view_key], ctypes.byref(v)))
        return 'mask' if (v.value & 1) else 'spans'

    def draw_records(self):
        """The frames' draw records as the last launch left them (include/moog_engine.h moog_engine_read_draw_records;
        csrc/moog_draw_record.h): (uint8 array [num_envs, stride], written_by_the_step_kernel).  Synchronises; for tests."""
        import numpy as np
        stride, in_step = ctypes.c_int64(), ctypes.c_int32()
        _engine.check(self._lib, self._lib.moog_engine_read_draw_records(self._handle, None, 0, ctypes.byref(stride), ctypes.byref(in_step)))
        out = np.zeros((self.num_envs, stride.value), np.uint8)
        with self._torch.cuda.device(self.device):
            _engine.check(self._lib, self._lib.moog_engine_read_draw_records(
                self._handle, ctypes.c_void_p(out.ctypes.data), out.nbytes, ctypes.byref(stride), ctypes.byref(in_step)))
        return out, bool(in_step.value)

    def raster_compact_edges(self):
        """Whether the mask rasteriser keeps this program's edge records in their 4-byte form (csrc/moog_raster_mask_core.h
        RmEdgesCompact: picked when the 16-byte records would keep frames off a CU; MOOG_RASTER_COMPACT=0 / 1 forces)."""
        v = ctypes.c_int32()
        _engine.check(self._lib, self._lib.moog_engine_raster_path(self._handle, ctypes.byref(v)))
        return v.value == 3

    # -- plumbing ---------------------------------------------------------------------
    def _stream(self):
        return ctypes.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _inject(self, uniforms):
        if uniforms is None:
            return None, None
        t = self._torch.as_tensor(uniforms, dtype=self._torch.float64, device=self.device).contiguous()
        assert t.dim() == 2 and t.shape[0] == self.num_envs
        inj = _abi.Inject()
        inj.uniforms = ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_double))
        inj.per_env = t.shape[1]
        return inj, t

    def _timestep(self):
        return dm_env.TimeStep(self.step_type, self.reward, self.discount, self._observation())

    def _observation(self):
        from .observers import raw_state
        obs = {}
        for key, o in self.observers.items():   # the reference's dict order
            if isinstance(o, raw_state.RawState):
                obs[key] = raw_state.StateView(self)
            elif key in self.tables:
                obs[key] = self.tables[key]
            else:
                obs[key] = self._frames[key]
        return obs


    def _poll_faults(self):
        if not self.check_faults:
            return
        bits = ctypes.c_int32()
        _engine.check(self._lib, self._lib.moog_engine_poll_faults(self._handle, 0, ctypes.byref(bits)))
        if bits.value:
            self._torch.cuda.synchronize(self.device)
            self.raise_faults()

    def clear_faults(self):
        """Forgets the recorded faults (the per-env fault words and the engine's summary word)."""
        self._torch.cuda.synchronize(self.device)
        self.state_i32[:, self.layout.o_fault] = 0
        bits = ctypes.c_int32()
        _engine.check(self._lib, self._lib.moog_engine_poll_faults(self._handle, 1, ctypes.byref(bits)))

    def layer_usage(self):
        """Usage of the layers that rules append to (the reference's unbounded lists; here `layer_capacity` slots):
        {layer: dict(capacity=, high_water=, dropped=)} over all envs and calls since the environment was made --
        high_water is the most sprites an append ever needed room for (capacity + 1 once the layer overflowed), dropped
        the appends that found the layer full.  The sizing hint for `layer_capacity`.  Synchronises the device."""
        P = self.compiled.program
        hw = (ctypes.c_int32 * _abi.MOOG_MAX_LAYERS)()
        dr = (ctypes.c_int32 * _abi.MOOG_MAX_LAYERS)()
        self._torch.cuda.synchronize(self.device)
        _engine.check(self._lib, self._lib.moog_engine_layer_usage(self._handle, hw, dr))
        return {name: dict(capacity=int(P.layer_nslots[li]), high_water=int(hw[li]), dropped=int(dr[li]))
                for li, name in enumerate(self.compiled.layer_names) if P.layer_dynamic[li]}

    def _grow_if_close(self):
        """layer_capacity='auto': grows the layers whose high-water mark has come close to their capacity -- within a quarter of
        it: the layer is doubled; after fit_layer_capacity(headroom=h), within h / 2 of it: the layer grows by the factor 1 + h.
        Nothing has been dropped at that point (a dropped append raises, as ever), so the state moves over intact."""
        import math
        m = getattr(self, '_grow_margin', 0.25)
        factor = 2.0 if m >= 0.25 else 1.0 + 2.0 * m
        use = self.layer_usage()
        grow = {name: max(int(math.ceil(factor * u['capacity'])), u['high_water'] + 4) for name, u in use.items()
                if u['dropped'] == 0 and u['capacity'] - u['high_water'] <= max(2.0 if m < 0.25 else 0.0, m * u['capacity'])}
        if grow:
            self._grow_layers(grow)

    def fit_layer_capacity(self, headroom=0.25, min_room=4):
        """Sizes the layers that rules append to by what the batch has needed so far instead of by their capacity: every such
        layer gets `high-water mark x (1 + headroom)` slots (at least `min_room` more than the mark, never fewer than the last
        slot in use in any env), the engine is re-created and the records move over as in _grow_layers.  From then on the
        layers grow on demand (layer_capacity='auto').  A state record holds every slot's vertices, so its size -- and with it
        how many envs share a CU's LDS in the step kernel -- follows the capacities: first_person_predators_prey at
        {'prey': 32, 'predators': 96} is one env per CU, fitted to a 4096-env batch's needs it is two or three.
        Returns the new capacities ({} when nothing shrinks).  Results do not depend on capacities (a sprite keeps its layer
        and its place in the layer's list)."""
        import math
        if self._action_repeat > 1:
            raise NotImplementedError('fit_layer_capacity turns growth on demand on (layer_capacity=\'auto\'), whose margin is sized '
                                      'for one env-step of appends per call: set_action_repeat(1) first')
        torch = self._torch
        P, L = self.compiled.program, self.layout
        use = self.layer_usage()
        flags = self.state_i32[:, L.o_flags:L.o_flags + L.S] & 1
        caps = {}
        for li, name in enumerate(self.compiled.layer_names):
            if name not in use:
                continue
            s0, n_old = int(P.layer_slot0[li]), int(P.layer_nslots[li])
            alive = flags[:, s0:s0 + n_old].any(dim=0).nonzero()
            in_use = int(alive.max().item()) + 1 if alive.numel() else 0
            mark = max(use[name]['high_water'], in_use)
            # (never below the slots the initializer fills: a layer whose sprites have all vanished is re-made whole by the
            #  next reset, and compile_config refuses fewer slots than that)
            want = max(mark + int(min_room), int(math.ceil(mark * (1.0 + headroom))), 1, int(self.compiled.layer_n_init.get(name, 0)))
            if want < n_old:
                caps[name] = want
        if caps:
            self._grow_layers(caps)
            self._auto_capacity = True
            self._grow_margin = min(0.25, 0.5 * float(headroom))
        return caps

    def _grow_layers(self, new_caps):
        """Re-creates the engine with other capacities for the given layers ({layer: slots}; fewer slots only when the
        slots given up hold no sprite: fit_layer_capacity) and moves every env's state records to the new layout: a sprite keeps its layer and its position in the layer's list, everything that is not per
        slot (task / rule / action state, counters, the random streams' positions) is copied as is."""
        torch = self._torch
        old_c, old_L = self.compiled, self.layout
        old_P = old_c.program
        caps = {name: int(old_P.layer_nslots[li]) for li, name in enumerate(old_c.layer_names) if old_P.layer_dynamic[li]}
        caps.update({k: int(v) for k, v in new_caps.items()})
        new_c = _compiler.compile_config(*self._config_args, layer_capacity=caps, keep_sprite_factors=self._keep_sprite_factors)
        P, L = new_c.program, new_c.layout
        assert list(new_c.layer_names) == list(old_c.layer_names)
        # Other capacities = another program = another hash: the specialised step kernel of the old program does not fit.
        # specialize=True builds the new program's (~20 s of hipcc, once per capacity set; kept in the spec directory); otherwise the
        # engine falls back to the generic kernels -- said once, so that a slower run is not a mystery (step_kernel() tells).
        was_specialised = self.step_kernel() == 'specialised'
        if self._specialize:
            from . import _spec
            _spec.build(P)
        # index maps: for every word of a new record, the word of the old record it comes from (-1: zero)
        src_f = np.full(L.f64_per_env, -1, np.int64)
        src_q = np.full(L.i32_per_env, -1, np.int64)
        slot_map = []   # (old slot, new slot)
        for li in range(P.n_layers):
            o0, n_old, n0 = int(old_P.layer_slot0[li]), int(old_P.layer_nslots[li]), int(P.layer_slot0[li])
            slot_map += [(o0 + k, n0 + k) for k in range(min(n_old, int(P.layer_nslots[li])))]
        for name, width in (('o_pos', 2), ('o_vel', 2), ('o_angle', 1), ('o_angvel', 1), ('o_mass', 1), ('o_color', 3),
                            ('o_inertia', 2), ('o_maxr', 1), ('o_scale', 1), ('o_aspect', 1)):
            a, b = getattr(old_L, name), getattr(L, name)
            if a < 0 or b < 0:
                assert a < 0 and b < 0, name
                continue
            for so, sn in slot_map:
                src_f[b + width * sn:b + width * (sn + 1)] = np.arange(a + width * so, a + width * (so + 1))
        for so, sn in slot_map:   # vertices
            vo, vn, cap = int(old_P.slot_voff[so]), int(P.slot_voff[sn]), int(old_P.slot_vcap[so])
            assert int(P.slot_vcap[sn]) >= cap
            src_f[L.o_verts + 2 * vn:L.o_verts + 2 * (vn + cap)] = np.arange(old_L.o_verts + 2 * vo, old_L.o_verts + 2 * (vo + cap))
        n_act = 2 * max(1, int(P.n_actions))
        for name, count in (('o_action', n_act), ('o_task', int(P.n_tasks)), ('o_rule', int(P.n_rules)),
                            ('o_hdraw', int(P.n_hdraws)), ('o_rule2', int(P.n_rules))):
            a, b = getattr(old_L, name), getattr(L, name)
            if a >= 0 and b >= 0 and count > 0:
                src_f[b:b + count] = np.arange(a, a + count)
        for name in ('o_flags', 'o_nverts', 'o_opacity', 'o_shape', 'o_tele', 'o_valias', 'o_fmask'):
            a, b = getattr(old_L, name), getattr(L, name)
            if a < 0 or b < 0:
                assert a < 0 and b < 0, name
                continue
            for so, sn in slot_map:
                src_q[b + sn] = a + so
        for name, count in (('o_step_count', 1), ('o_reset_next', 1), ('o_fault', 1), ('o_rng', 4),
                            ('o_maze', _abi.MOOG_MAX_MAZE + _abi.MOOG_MAX_MAZE_POINTS)):
            a, b = getattr(old_L, name), getattr(L, name)
            if a >= 0 and b >= 0:
                src_q[b:b + count] = np.arange(a, a + count)
        torch.cuda.synchronize(self.device)
        with torch.cuda.device(self.device):
            def move(old, src, dtype):
                idx = torch.as_tensor(np.where(src < 0, 0, src), device=self.device)
                keep = torch.as_tensor(src >= 0, device=self.device)
                new = old.index_select(1, idx)
                return torch.where(keep.unsqueeze(0), new, torch.zeros((), dtype=dtype, device=self.device)).contiguous()
            new_f = move(self.state_f64, src_f, torch.float64)
            new_q = move(self.state_i32, src_q, torch.int32)
            # the new engine, over the new records (outputs stay where they are)
            had_schedule, f32 = self._perm is not None, self._action_f32
            self.close()
            self.compiled, self.layout = new_c, L
            self.state_f64, self.state_i32 = new_f, new_q
            # (other capacities, other row counts: new tensors for the tables, sensors and contacts -- their rows and ids move
            #  -- filled from the records that have just moved over, the readings under the new ids at once; the views' and
            #  segmentations' tensors keep their size)
            self.tables = self.allocate_table_buffers(torch, new_c, self.num_envs, self.device)
            self._open_engine()
            self._observe_tables()
            if f32:
                _engine.check(self._lib, self._lib.moog_engine_set_action_dtype(self._handle, 1))
            self._apply_action_repeat()
        if had_schedule:
            self.enable_cost_schedule(True)
        self._apply_reset_pool()
        self._setup_color_fn()
        if self.compiled.segmentations:   # (the masks under the new ids at once, like the tables: drawn with the frames)
            self.observation()
        self.capacity_growths = getattr(self, 'capacity_growths', []) + [dict(caps)]
        if was_specialised and self.step_kernel() != 'specialised' and not getattr(self, '_warned_generic', False):
            self._warned_generic = True
            import warnings
            warnings.warn('layer capacities changed to %s: the program-specialised step kernel was built for the old capacities, '
                          'the generic step kernel is in use from here on (BatchedEnvironment(specialize=True) or '
                          '`moog._spec.build(env.compiled.program)` builds one for the new program)' % (dict(caps),), RuntimeWarning)

    def raise_faults(self):
        """Re-raises device-side per-env faults with the reference's exception types.

        Faults are STICKY, like a broken environment in the reference: the per-env fault words (and the engine's summary
        word that _poll_faults reads) stay set, so every later reset() / step() / observation() raises again until
        clear_faults() -- after which the faulted envs should be reset."""
        faults = self.state_i32[:, self.layout.o_fault]
        if not bool((faults != 0).any().item()):
            return
        allbits = 0
        for v in faults.unique().tolist():
            allbits |= int(v)
        for bit, exc, msg in _FAULT_EXC:
            if allbits & bit:
                env = int((faults & bit).nonzero()[0].item())
                if bit == _abi.MOOG_FAULT_LAYER_FULL:   # which layer, and how much room it asked for
                    full = {k: v for k, v in self.layer_usage().items() if v['dropped'] > 0}
                    msg += ' Overflowing layers: %s -- pass layer_capacity={layer: slots} with more than high_water ' \
                           'slots (the reference\'s lists are unbounded; env.layer_usage() reports the demand).' % (full,)
                raise exc('%s (env %d)' % (msg, env))

    # -- dm_env surface (environment.py:82-131) ------------------------------------------
    def reset(self, env_mask=None, injected_uniforms=None):
        self._poll_faults()
        mask_t = None
        mask_ptr = None
        if env_mask is not None:
            mask_t = self._torch.as_tensor(env_mask, device=self.device).to(self._torch.uint8).contiguous()
            mask_ptr = ctypes.c_void_p(mask_t.data_ptr())
        inj, keep = self._inject(injected_uniforms)
        with self._torch.cuda.device(self.device):
            _engine.check(self._lib, self._lib.moog_engine_reset(
                self._handle, mask_ptr, ctypes.byref(inj) if inj else None,
                ctypes.byref(self._out if self._color_fn is None else self._out_noimg), self._stream()))
        if self._color_fn is not None:
            self._render_with_colors()
        if mask_t is None:
            self.repeat_count.zero_()
        else:
            self.repeat_count.masked_fill_(mask_t.bool(), 0)
        if self.check_faults:
            self.raise_faults()   # (a reset is rare and its sampler is where most faults come from: check at once)
        del keep, mask_t
        self._host_reset()
        return self._timestep()

    def step(self, action, injected_uniforms=None):
        torch = self._torch
        if injected_uniforms is not None and self._action_repeat > 1:
            raise NotImplementedError('injected_uniforms feed ONE env-step (a per-call stream); action_repeat=%d takes several per '
                                      'call: set_action_repeat(1) for the injected calls' % self._action_repeat)
        self._poll_faults()
        if self._composite:
            a = self._pack_composite(action)
        elif self._is_grid:
            a = torch.as_tensor(action, device=self.device).to(torch.int32).contiguous()
            assert a.shape == (self.num_envs,)
        else:
            a = torch.as_tensor(action, device=self.device)
            # float32 actions -- the dtype of the reference's Joystick spec (joystick.py:42-43) -- stay float32: the
            # reference then multiplies by scaling_factor in float32, and so does the engine
            f32 = a.dtype == torch.float32
            if f32 != self._action_f32:
                _engine.check(self._lib, self._lib.moog_engine_set_action_dtype(self._handle, 1 if f32 else 0))
                self._action_f32 = f32
            a = (a if f32 else a.to(torch.float64)).contiguous()
            assert a.shape == (self.num_envs, 2)
        self._step_host_rules()
        inj, keep = self._inject(injected_uniforms)
        with torch.cuda.device(self.device):
            _engine.check(self._lib, self._lib.moog_engine_step(
                self._handle, ctypes.c_void_p(a.data_ptr()), ctypes.byref(inj) if inj else None,
                ctypes.byref(self._out if self._color_fn is None else self._out_noimg), self._stream()))
        if self._color_fn is not None:
            self._render_with_colors()
        self._last_action = a
        self._after_step_call(injected_uniforms is not None)
        del keep
        return self._timestep()

    def _step_host_rules(self):
        if self._host_rules or self._meta_state_initializer is not None:
            # environment.py:100-104: an auto-reset re-initialises the meta-state; either way
            # every rule steps once per call
            flags = self.reset_next_step.cpu().numpy()
            if self.num_envs == 1:
                if flags[0]:
                    self._host_reset()
                else:
                    for r in self._host_rules:
                        r.step(None, self._meta_state)
            else:
                if self._meta_state is None:   # stepped from a loaded state without a reset()
                    self._meta_state = [self._new_meta_state() for _ in range(self.num_envs)]
                for i in range(self.num_envs):
                    if flags[i]:
                        self._meta_state[i] = self._new_meta_state()
                    for r in self._host_rules:
                        r.step(None, self._meta_state[i])

    def _after_step_call(self, injected):
        # Programs whose rules append to layers can overflow a layer's capacity at any step:
        # surface that (one host sync per step; set check_faults = False to opt out).
        if self.check_faults == 'sync' or (self.check_faults and (injected or self._dynamic_layers)):
            self.raise_faults()
        if self._auto_capacity and self._dynamic_layers:
            self._n_step_calls += 1
            if self._fit_after > 0 and self._n_step_calls == self._fit_after:
                self.fit_layer_capacity()   # (once; sets the margin _grow_if_close works with from here on)
            self._grow_if_close()

    # -- open-loop rollouts (include/moog_engine.h moog_engine_step_sequence) -----------------
    def _sequence_shape(self, n):
        """The shape of a rollout's actions for n envs, as the error messages name it."""
        if self._composite:
            return '[T, %d, %d, 2] (or a dict {key: [T, %d, 2] / [T, %d]} with the keys %s)' % (
                n, len(self.action_space.action_keys), n, n, list(self.action_space.action_keys))
        return '[T, %d]' % n if self._is_grid else '[T, %d, 2]' % n

    def _pack_sequence(self, actions, n=None, _blocks=False):
        """A rollout's actions as ONE device tensor [T, n, ...], step t's block laid out as step() hands one to the engine
        (float32 Joystick actions stay float32).  ValueError: a shape or a dict key that does not fit, T out of range.
        (_blocks: any number of blocks -- _pack_candidates packs its K x T of them here and checks the two ranges itself.)"""
        torch = self._torch
        n = self.num_envs if n is None else n

        def bad(got):
            return ValueError('rollout: actions of shape %s, expected %s with 1 <= T <= %d'
                              % (got, self._sequence_shape(n), _abi.MOOG_MAX_ACTION_REPEAT))

        def shape_of(v):
            return tuple(v.shape) if hasattr(v, 'shape') else tuple(np.shape(v))

        if self._composite:
            keys = list(self.action_space.action_keys)
            if isinstance(actions, dict):
                if set(actions) != set(keys):
                    raise ValueError('rollout: composite action keys %s, expected %s, each [T, %d, 2] or [T, %d]'
                                     % (sorted(actions), keys, n, n))
                vs = [torch.as_tensor(actions[key], device=self.device).to(torch.float64) for key in keys]
                T = vs[0].shape[0] if vs[0].dim() >= 2 else -1
                a = torch.zeros((max(T, 0), n, len(keys), 2), dtype=torch.float64, device=self.device)
                for i, v in enumerate(vs):
                    if tuple(v.shape) == (T, n):   # Grid move indices
                        a[:, :, i, 0] = v
                    elif tuple(v.shape) == (T, n, 2):
                        a[:, :, i, :] = v
                    else:
                        raise bad({key: shape_of(actions[key]) for key in keys})
            else:
                a = torch.as_tensor(actions, device=self.device).to(torch.float64)
                if a.dim() != 4 or tuple(a.shape[1:]) != (n, len(keys), 2):
                    raise bad(tuple(a.shape))
            if self._n_actions == 1:   # a Composite of one space is that space's own buffer (_pack_composite)
                a = a[:, :, 0, :]
                a = a[:, :, 0].to(torch.int32) if self.compiled.program.action.kind == _abi.MOOG_ACTION_GRID else a
            else:
                a = a.reshape(a.shape[0], n, 2 * self._n_actions)
        elif self._is_grid:
            a = torch.as_tensor(actions, device=self.device)
            if a.dim() != 2 or a.shape[1] != n:
                raise bad(tuple(a.shape))
            a = a.to(torch.int32)
        else:
            a = torch.as_tensor(actions, device=self.device)
            if a.dim() != 3 or tuple(a.shape[1:]) != (n, 2):
                raise bad(tuple(a.shape))
            a = a if a.dtype == torch.float32 else a.to(torch.float64)
        if not _blocks and not 1 <= a.shape[0] <= _abi.MOOG_MAX_ACTION_REPEAT:
            raise bad(tuple(a.shape))
        return a if a[0].is_contiguous() and (a.shape[0] == 1 or a.stride(0) >= a[0].numel()) else a.contiguous()

    @staticmethod
    def _sequence_length(actions):
        if isinstance(actions, dict):
            actions = next(iter(actions.values())) if actions else ()
        return len(actions)

    def _check_rollout(self, T):
        """T as an int, or the reason this engine cannot run a sequence of T env-steps inside one launch."""
        if not 1 <= T <= _abi.MOOG_MAX_ACTION_REPEAT:
            raise ValueError('rollout: T = %d actions per env, expected 1 .. %d' % (T, _abi.MOOG_MAX_ACTION_REPEAT))
        if self._action_repeat > 1:
            raise NotImplementedError('rollout on an engine with action_repeat=%d (a hold count per sequence entry) is not '
                                      'available: set_action_repeat(1) first' % self._action_repeat)
        return self._check_action_repeat(T)   # (T env-steps inside one launch: what a repeat of T cannot do, this cannot either)

    def _check_record(self, record):
        """rollout()'s `record` as a list of SpriteTable keys, or the reason it cannot be recorded (no device needed)."""
        keys = [record] if isinstance(record, str) else list(record)
        if not keys:
            raise ValueError('rollout: record is empty: name at least one SpriteTable observer of the config (or pass None)')
        for key in keys:
            if key not in self.observers:
                raise KeyError('rollout: record names %r, which is not an observer of this config (%s)'
                               % (key, sorted(self.observers, key=str)))
            if not isinstance(self.observers[key], sprite_table.SpriteTable):
                raise TypeError('rollout: record names %r, a %s: only SpriteTable observers are recorded per step'
                                % (key, type(self.observers[key]).__name__))
        if len(set(keys)) != len(keys):
            raise ValueError('rollout: record names a key twice: %s' % (keys,))
        return keys

    def _new_trajectory(self, keys, T, n=None):
        """{key: [T, n, rows, columns] of the table's dtype}, uninitialised: the step kernel writes every element."""
        torch = self._torch
        n = self.num_envs if n is None else n
        with torch.cuda.device(self.device):
            return {key: torch.empty((T, n) + tuple(self.tables[key].shape[1:]), dtype=self.tables[key].dtype, device=self.device)
                    for key in keys}

    def rollout(self, actions, record=None):
        """Open loop: T env-steps with T different actions inside one launch of the step kernel, no observation in between
        (a planner's roll-out: random shooting, CEM / MPC, the leaves of a tree search; with snapshot() / restore(), the
        reference's SimulationEnvironment).  actions: [T, N, 2] (Joystick; float32 stays float32, as in step()), [T, N]
        (Grid), [T, N, n_spaces, 2] or a dict of [T, N, 2] / [T, N] (Composite); numpy or device tensors, 1 <= T <=
        MOOG_MAX_ACTION_REPEAT.  Returns (timestep, rewards, count):
          rewards   float64 [T, N]: the reward of every env-step; 0.0 for the steps an env did not take (those behind the
                    step that ended its episode, every step of an env the call reset instead)
          count     `repeat_count`, int32 [N]: the env-steps each env took (0: the call reset the env, a FIRST timestep)
          timestep  what a step() at action_repeat=T returns: the rewards' sum in step order, the step_type / discount of
                    the last step taken, the observations after it.
        The state after the call is, bit for bit, the state after count single step() calls with the same actions.
        record: the key of a SpriteTable observer of the config, or a list / tuple of keys: the states in between.  The call
        then returns (timestep, rewards, count, trajectory), trajectory = {key: a fresh tensor [T, N, rows, columns] of the
        table's dtype}: trajectory[key][j, e] holds exactly what tables[key][e] would hold after a step() call that took
        env-step j of env e (the step that ended an episode included), and zero bits -- `alive` too -- for the steps env e
        did not take.  The step kernel writes it from the record on chip (moog_engine_set_table_trajectory)."""
        keys = None if record is None else self._check_record(record)   # (refusals first: they need no device)
        T = self._check_rollout(self._sequence_length(actions))
        torch = self._torch
        a = self._pack_sequence(actions)
        with torch.cuda.device(self.device):
            rewards = torch.empty((T, self.num_envs), dtype=torch.float64, device=self.device)
        if keys is None:
            ts = self._rollout_packed(a, rewards)
            return ts, rewards, self.repeat_count
        traj = self._new_trajectory(keys, T)
        ts = self._rollout_packed(a, rewards, traj)
        return ts, rewards, self.repeat_count, traj

    def _bind_trajectory(self, traj):
        """Binds (or, with None for a tensor, unbinds) the trajectory tensors of the sequences to come."""
        for key, t in traj.items():
            _engine.check(self._lib, self._lib.moog_engine_set_table_trajectory(
                self._handle, self._table_index[key], ctypes.c_void_p(t.data_ptr() if t is not None else None),
                t.stride(0) if t is not None else 0))

    def _rollout_packed(self, a, rewards, traj=None):
        """rollout() on packed actions [T, n, ...] and a reward tensor [T, n] of the caller's, either one possibly a slice of
        a whole batch's (rows further apart than their length: the engine takes the two strides).  traj: None, or {SpriteTable
        key: [T, n, rows, columns]} of the caller's, likewise possibly slices (the blocks of two steps further apart than n
        envs' rows): recorded by this call only -- the tensors are bound before it and unbound behind it."""
        torch = self._torch
        T = self._check_rollout(int(a.shape[0]))
        assert a.shape[1] == self.num_envs and a[0].is_contiguous(), (tuple(a.shape), a.stride())
        assert tuple(rewards.shape) == (T, self.num_envs) and rewards.dtype == torch.float64 and rewards.stride(1) == 1
        for key, t in (traj or {}).items():
            own = self.tables[key]
            assert tuple(t.shape) == (T, self.num_envs) + tuple(own.shape[1:]) and t.dtype == own.dtype, (key, tuple(t.shape), t.dtype)
            assert t[0].is_contiguous() and t.stride(0) >= t[0].numel(), (key, t.stride())   # (the inner three dimensions)
        self._poll_faults()
        if a.dtype != torch.int32 and not self._composite:
            f32 = a.dtype == torch.float32
            if f32 != self._action_f32:
                _engine.check(self._lib, self._lib.moog_engine_set_action_dtype(self._handle, 1 if f32 else 0))
                self._action_f32 = f32
        self._step_host_rules()   # (T == 1: _check_rollout refuses host-side rules beyond that)
        if traj:
            self._bind_trajectory(traj)
        try:
            with torch.cuda.device(self.device):
                _engine.check(self._lib, self._lib.moog_engine_step_sequence(
                    self._handle, ctypes.c_void_p(a.data_ptr()), T, a.stride(0) * a.element_size(),
                    ctypes.c_void_p(rewards.data_ptr()), rewards.stride(0), None,
                    ctypes.byref(self._out if self._color_fn is None else self._out_noimg), self._stream()))
        finally:
            if traj:   # (a later rollout() without `record` must not write to this call's tensors)
                self._bind_trajectory(dict.fromkeys(traj))
        if self._color_fn is not None:
            self._render_with_colors()
        self._last_action = a
        self._after_step_call(False)
        return self._timestep()

    # -- candidate rollouts (include/moog_engine.h moog_engine_plan_sequences) -----------------
    def plan_kernel(self):
        """'specialised' when rollout_candidates runs a kernel compiled for this program (moog/_spec.py), else 'generic'."""
        v = ctypes.c_int32()
        _engine.check(self._lib, self._lib.moog_engine_plan_kernel(self._handle, ctypes.byref(v)))
        return 'specialised' if v.value else 'generic'

    @staticmethod
    def _candidate_dims(actions):
        """(K, T) of rollout_candidates' actions, from their shape alone."""
        if isinstance(actions, dict):
            actions = next(iter(actions.values())) if actions else ()
        shape = tuple(actions.shape) if hasattr(actions, 'shape') else tuple(np.shape(actions))
        if len(shape) < 3:
            raise ValueError('rollout_candidates: actions of shape %s, expected a leading [K, T, num_envs]' % (shape,))
        return int(shape[0]), int(shape[1])

    def _check_candidates(self, K, T):
        """(K, T), or the reason this engine cannot evaluate K sequences of T env-steps per env inside one launch."""
        if not 1 <= K <= _abi.MOOG_MAX_PLAN_CANDIDATES:
            raise ValueError('rollout_candidates: K = %d candidates per env, expected 1 .. %d' % (K, _abi.MOOG_MAX_PLAN_CANDIDATES))
        return K, self._check_rollout(T)

    def _pack_candidates(self, actions, n=None):
        """rollout_candidates' actions as ONE contiguous device tensor [K, T, n, ...], block [k, t] laid out as step() hands
        one to the engine (_pack_sequence over the K x T blocks)."""
        torch = self._torch
        n = self.num_envs if n is None else n
        K, T = self._candidate_dims(actions)

        def flat(v):
            v = torch.as_tensor(v, device=self.device)
            return v.reshape((K * T,) + tuple(v.shape[2:])) if v.dim() >= 2 and tuple(v.shape[:2]) == (K, T) else v

        try:
            a = self._pack_sequence({key: flat(v) for key, v in actions.items()} if isinstance(actions, dict) else flat(actions),
                                    n, _blocks=True)
        except ValueError as err:
            if 'composite action keys' in str(err):
                raise
            got = ({key: tuple(np.shape(v)) if not hasattr(v, 'shape') else tuple(v.shape) for key, v in actions.items()}
                   if isinstance(actions, dict) else (tuple(actions.shape) if hasattr(actions, 'shape') else tuple(np.shape(actions))))
            raise ValueError('rollout_candidates: actions of shape %s, expected %s with 1 <= K <= %d and 1 <= T <= %d'
                             % (got, self._sequence_shape(n).replace('[T, ', '[K, T, '), _abi.MOOG_MAX_PLAN_CANDIDATES,
                                _abi.MOOG_MAX_ACTION_REPEAT)) from None
        a = a.contiguous()
        return a.reshape((K, T) + tuple(a.shape[1:]))

    def _new_candidate_outputs(self, K, T, keys, n=None):
        """(rewards [K, T, n] float64, count [K, n] int32, ended [K, n] uint8, {key: [K, T, n, rows, columns]} or None),
        uninitialised: the candidate kernel writes every element."""
        torch = self._torch
        n = self.num_envs if n is None else n
        with torch.cuda.device(self.device):
            rewards = torch.empty((K, T, n), dtype=torch.float64, device=self.device)
            count = torch.empty((K, n), dtype=torch.int32, device=self.device)
            ended = torch.empty((K, n), dtype=torch.uint8, device=self.device)
            traj = None if keys is None else {
                key: torch.empty((K, T, n) + tuple(self.tables[key].shape[1:]), dtype=self.tables[key].dtype, device=self.device)
                for key in keys}
        return rewards, count, ended, traj

    def rollout_candidates(self, actions, record=None):
        """A planner's inner loop (random shooting, CEM / MPC): K action sequences of T env-steps for every env, all from the
        env's present state, in ONE launch of a step kernel that reads each record K times and writes none back.
        actions: rollout()'s layouts with a leading K -- [K, T, N, 2] (Joystick; float32 stays float32), [K, T, N] (Grid),
        [K, T, N, n_spaces, 2] or a dict of [K, T, N, 2] / [K, T, N] (Composite); 1 <= T <= MOOG_MAX_ACTION_REPEAT,
        1 <= K <= MOOG_MAX_PLAN_CANDIDATES.  Returns (rewards, count, ended):
          rewards   float64 [K, T, N]: the reward of every env-step candidate k took in env e; 0.0 for the steps not taken
          count     int32 [K, N]: the env-steps taken
          ended     uint8 [K, N]: 1 when the candidate's last step taken asked for a reset
        With record (a SpriteTable key or a list of keys, as in rollout()) a fourth value, trajectory = {key: a fresh tensor
        [K, T, N, rows, columns] of the table's dtype}: block [k, j, e] is what rollout(actions[k], record=key) would put
        in [j, e], zero bits for the steps not taken.
        Candidate k's outputs equal, bit for bit, those of rollout(actions[k]) issued on this state.  The state (both
        tensors, random counters included) is put back afterwards, and the call changes nothing.
        So: an env whose reset_next is set takes no step in any candidate (count 0, rewards 0.0, ended 0) and is not reset --
        the next real step() does that as always; the candidates read the record's random counters as they stand, so all K
        see the same draws (common random numbers) and the real step that follows sees them too; host-side meta-state
        rules do not run.  Refused, before anything touches a device and with rollout()'s error types: shapes that do not
        fit, K or T out of range, action_repeat above 1, host-side rules with T > 1, layer_capacity='auto', record keys
        that are no SpriteTable of the config."""
        keys = None if record is None else self._check_record(record)   # (refusals first: they need no device)
        K, T = self._check_candidates(*self._candidate_dims(actions))
        a = self._pack_candidates(actions)
        rewards, count, ended, traj = self._new_candidate_outputs(K, T, keys)
        self._rollout_candidates_packed(a, rewards, count, ended, traj)
        return (rewards, count, ended) if keys is None else (rewards, count, ended, traj)

    def _rollout_candidates_packed(self, a, rewards, count, ended, traj=None):
        """rollout_candidates() on packed actions [K, T, n, ...] and outputs of the caller's -- rewards [K, T, n], count and
        ended [K, n], traj None or {SpriteTable key: [K, T, n, rows, columns]} -- any of them possibly a slice of a whole
        batch's along the env axis: the engine takes the strides.  The trajectory tensors are bound before the call and
        unbound behind it, as _rollout_packed does."""
        torch = self._torch
        K, T = self._check_candidates(int(a.shape[0]), int(a.shape[1]))
        n = self.num_envs
        assert a.shape[2] == n and a[0, 0].is_contiguous(), (tuple(a.shape), a.stride())
        assert tuple(rewards.shape) == (K, T, n) and rewards.dtype == torch.float64 and rewards.stride(2) == 1
        assert tuple(count.shape) == (K, n) and count.dtype == torch.int32 and count.stride(1) == 1
        assert tuple(ended.shape) == (K, n) and ended.dtype == torch.uint8 and ended.stride() == count.stride()
        strides = (ctypes.c_int64 * _abi.MOOG_MAX_TABLES)()
        for key, t in (traj or {}).items():
            own = self.tables[key]
            assert tuple(t.shape) == (K, T, n) + tuple(own.shape[1:]) and t.dtype == own.dtype, (key, tuple(t.shape), t.dtype)
            assert t[0, 0].is_contiguous() and t.stride(1) >= t[0, 0].numel(), (key, t.stride())
            strides[self._table_index[key]] = t.stride(0)
        if a.dtype != torch.int32 and not self._composite:
            f32 = a.dtype == torch.float32
            if f32 != self._action_f32:
                _engine.check(self._lib, self._lib.moog_engine_set_action_dtype(self._handle, 1 if f32 else 0))
                self._action_f32 = f32
        if traj:
            for key, t in traj.items():
                _engine.check(self._lib, self._lib.moog_engine_set_table_trajectory(
                    self._handle, self._table_index[key], ctypes.c_void_p(t.data_ptr()), t.stride(1)))
        try:
            with torch.cuda.device(self.device):
                _engine.check(self._lib, self._lib.moog_engine_plan_sequences(
                    self._handle, ctypes.c_void_p(a.data_ptr()), K, T, a.stride(0) * a.element_size(), a.stride(1) * a.element_size(),
                    ctypes.c_void_p(rewards.data_ptr()), rewards.stride(0), rewards.stride(1),
                    ctypes.c_void_p(count.data_ptr()), ctypes.c_void_p(ended.data_ptr()), count.stride(0),
                    strides if traj else None, self._stream()))
        finally:
            if traj:   # (a later call without `record` must not write to this call's tensors)
                self._bind_trajectory(dict.fromkeys(traj))

    def _pack_composite(self, action):
        """Composite actions (composite.py:51-62): a dict {key: tensor [N, 2] or, for a Grid
        sub-space, [N] move indices}, or the packed f64 tensor [N, n_spaces, 2] itself."""
        torch = self._torch
        n, k = self.num_envs, self._n_actions
        if isinstance(action, dict):
            keys = self.action_space.action_keys
            if set(action) != set(keys):
                raise KeyError('composite action keys %s, expected %s' % (sorted(action), keys))
            a = torch.zeros((n, len(keys), 2), dtype=torch.float64, device=self.device)
            for i, key in enumerate(keys):
                v = torch.as_tensor(action[key], device=self.device).to(torch.float64)
                if v.dim() == 1 and v.shape[0] == n:      # Grid move indices
                    a[:, i, 0] = v
                else:
                    a[:, i, :] = v.reshape(n, 2)
        else:
            a = torch.as_tensor(action, device=self.device).to(torch.float64)
        a = a.reshape(n, -1)
        if self._n_actions == 1:   # a Composite of one space is that space's own buffer
            a = a[:, :2]
            if self.compiled.program.action.kind == _abi.MOOG_ACTION_GRID:
                return a[:, 0].to(torch.int32).contiguous()
            return a.contiguous()
        assert a.shape == (n, 2 * k), a.shape
        return a.contiguous()

    def _new_meta_state(self):
        return self._meta_state_initializer() if self._meta_state_initializer is not None else None

    def _host_reset(self):
        if self.num_envs == 1:
            self._meta_state = self._new_meta_state()
            for r in self._host_rules:
                r.step(None, self._meta_state)
            return
        self._meta_state = [self._new_meta_state() for _ in range(self.num_envs)]
        for m in self._meta_state:
            for r in self._host_rules:
                r.step(None, m)

    @property
    def meta_state(self):
        return self._meta_state

    # -- snapshot / restore (env_wrappers/simulation.py:64-91) ---------------------------------
    def snapshot(self):
        """Everything the reference's SimulationEnvironment deep-copies (state, action-space
        memory, task / rule counters, step_count, reset_next_step) lives in the two state
        records: a snapshot is a copy of them plus the host meta-state."""
        import copy
        return {'f64': self.state_f64.clone(), 'i32': self.state_i32.clone(),
                'meta_state': copy.deepcopy(self._meta_state)}

    def restore(self, snap):
        """Restores a snapshot.  The per-env random draw counters keep running (the
        reference does not rewind numpy's global RNG either), so repeated
        sim_step / sim_pop cycles sample different continuations."""
        o = self.layout.o_rng
        rng = self.state_i32[:, o:o + 4].clone()
        self.state_f64.copy_(snap['f64'])
        self.state_i32.copy_(snap['i32'])
        self.state_i32[:, o:o + 4] = rng
        self._meta_state = snap['meta_state']

    def physics_step(self, injected_uniforms=None):
        """`env.physics.step(env.state)` (tests/runtime_benchmark.py:101-107)."""
        inj, keep = self._inject(injected_uniforms)
        with self._torch.cuda.device(self.device):
            _engine.check(self._lib, self._lib.moog_engine_physics_only(
                self._handle, ctypes.byref(inj) if inj else None, self._stream()))
        del keep

    def observation(self):
        """Renders the current state (environment.py:128-131)."""
        self._poll_faults()
        self._observe_tables()
        if self._color_fn is not None:
            self._render_with_colors()
            return self._observation()
        if self.compiled.observer_key is None:   # (no PILRenderer: nothing to draw)
            return self._observation()
        with self._torch.cuda.device(self.device):
            _engine.check(self._lib, self._lib.moog_engine_render(
                self._handle, ctypes.c_void_p(self.image.data_ptr()), self._stream()))
        return self._observation()

    def observation_spec(self):
        from .observers import raw_state
        # (a SpriteTable's shape follows from this environment's layer capacities, a Contacts observer's too: the specs of the
        #  lowered kinds come from their descriptors.  A PILRenderer states its own, the reference's image_size + (3,).)
        lowered = {key: kind.spec(desc) for kind in OBSERVER_KINDS if kind.field != 'views'
                   for key, desc in getattr(self.compiled, kind.field)}
        return {k: lowered[k] if k in lowered else o.observation_spec()
                for k, o in self.observers.items() if not isinstance(o, raw_state.RawState)}

    def action_spec(self):
        return self.action_space.action_spec()

    def random_action(self):
        torch = self._torch
        if self._composite:
            out = {}
            for key, sub in self.action_space.action_spaces.items():
                kind = type(sub).__name__
                if kind == 'Grid':
                    out[key] = torch.randint(0, 5, (self.num_envs,), dtype=torch.int32, device=self.device)
                elif kind == 'SetPosition':
                    out[key] = torch.rand((self.num_envs, 2), dtype=torch.float64, device=self.device)
                else:
                    out[key] = torch.rand((self.num_envs, 2), dtype=torch.float64, device=self.device) * 2 - 1
            return out
        if self._is_grid:
            return torch.randint(0, 5, (self.num_envs,), dtype=torch.int32, device=self.device)
        return torch.rand((self.num_envs, 2), dtype=torch.float64, device=self.device) * 2 - 1

    @property
    def reset_next_step(self):
        return self.state_i32[:, self.layout.o_reset_next].bool()

    @property
    def step_count(self):
        return self.state_i32[:, self.layout.o_step_count]

    def static_prefix(self):
        """(number of leading sprite slots the rasteriser keeps as a cached picture, that
        picture uint8[H, W, 3] or None) -- include/moog_engine.h moog_engine_static_prefix."""
        n = ctypes.c_int32()
        _engine.check(self._lib, self._lib.moog_engine_static_prefix(self._handle, ctypes.byref(n), None, None))
        if n.value == 0:
            return 0, None
        img = self._torch.zeros_like(self.image[0])
        with self._torch.cuda.device(self.device):
            _engine.check(self._lib, self._lib.moog_engine_static_prefix(
                self._handle, ctypes.byref(n), ctypes.c_void_p(img.data_ptr()), self._stream()))
        return n.value, img

    def set_debug(self, step_debug=0, raster_stop=0):
        """Profiling aids of the kernels (include/moog_engine.h moog_engine_set_debug)."""
        _engine.check(self._lib, self._lib.moog_engine_set_debug(self._handle, int(step_debug), int(raster_stop)))

    # -- kernel timing -------------------------------------------------------------------
    def set_timing(self, enabled, kernels=None, every=1):
        """Brackets kernel launches with HIP events: all kernels, or only the MOOG_K_* ids in
        `kernels`; `every` = n brackets every n-th launch of a kernel (an event pair costs about
        5 microseconds of stream time, ~2 % of a step when every launch is bracketed)."""
        mask = 0
        if enabled:
            ids = range(_abi.MOOG_K_COUNT) if kernels is None else kernels
            for k in ids:
                mask |= 1 << int(k)
            mask |= (max(1, min(256, int(every))) - 1) << 8
        _engine.check(self._lib, self._lib.moog_engine_set_timing(self._handle, mask))

    def kernel_time(self, kernel_id):
        ms, cnt = ctypes.c_double(), ctypes.c_int64()
        _engine.check(self._lib, self._lib.moog_engine_kernel_time(
            self._handle, kernel_id, ctypes.byref(ms), ctypes.byref(cnt)))
        return ms.value, cnt.value

    # -- state views (sprite table as tensors) ----------------------------------------------
    def field(self, name):
        """Tensor view [N, S, ...] of one sprite field of the state record."""
        L, S = self.layout, self.layout.S
        f, q = self.state_f64, self.state_i32
        two = lambda o: f[:, o:o + 2 * S].view(-1, S, 2)
        one = lambda o: f[:, o:o + S]
        if name == 'position':
            return two(L.o_pos)
        if name == 'velocity':
            return two(L.o_vel)
        if name == 'angle':
            return one(L.o_angle)
        if name == 'angle_vel':
            return one(L.o_angvel)
        if name == 'mass':
            return one(L.o_mass)
        if name == 'color':
            return f[:, L.o_color:L.o_color + 3 * S].view(-1, S, 3)
        if name == 'inertia':
            return two(L.o_inertia)
        if name == 'max_radius':
            return one(L.o_maxr)
        if name == 'vertices':
            return f[:, L.o_verts:L.o_verts + 2 * L.TOTV].view(-1, L.TOTV, 2)
        if name == 'flags':
            return q[:, L.o_flags:L.o_flags + S]
        if name == 'alive':
            return (q[:, L.o_flags:L.o_flags + S] & _abi.MOOG_F_ALIVE).bool()
        if name == 'nverts':
            return q[:, L.o_nverts:L.o_nverts + S]
        if name == 'opacity':
            return q[:, L.o_opacity:L.o_opacity + S]
        raise KeyError(name)

    def sprites(self, env=0):
        """Host view of one env's state in the reference's shape (environment.py:143-146):
        OrderedDict layer name -> list of dicts with the Sprite.FACTOR_NAMES attributes
        (sprite.py:237-253), `vertices` and `slot`, live sprites in list order.  `scale` /
        `aspect_ratio` need `keep_sprite_factors=True` (else None)."""
        L, P, S = self.layout, self.compiled.program, self.layout.S
        f = self.state_f64[env].cpu().numpy()
        q = self.state_i32[env].cpu().numpy()
        out = collections.OrderedDict()
        for li, name in enumerate(self.compiled.layer_names):
            rows = []
            for s in range(P.layer_slot0[li], P.layer_slot0[li] + P.layer_nslots[li]):
                if not q[L.o_flags + s] & _abi.MOOG_F_ALIVE:
                    continue
                nv = int(q[L.o_nverts + s])
                o = L.o_verts + 2 * P.slot_voff[s]
                rows.append(dict(
                    x=float(f[L.o_pos + 2 * s]), y=float(f[L.o_pos + 2 * s + 1]),
                    shape=self.compiled.shape_names[int(q[L.o_shape + s])],
                    angle=float(f[L.o_angle + s]),
                    scale=float(f[L.o_scale + s]) if P.sprite_factors else None,
                    aspect_ratio=float(f[L.o_aspect + s]) if P.sprite_factors else None,
                    c0=float(f[L.o_color + 3 * s]), c1=float(f[L.o_color + 3 * s + 1]),
                    c2=float(f[L.o_color + 3 * s + 2]), opacity=int(q[L.o_opacity + s]),
                    x_vel=float(f[L.o_vel + 2 * s]), y_vel=float(f[L.o_vel + 2 * s + 1]),
                    angle_vel=float(f[L.o_angvel + s]), mass=float(f[L.o_mass + s]), metadata=None,
                    vertices=f[o:o + 2 * nv].reshape(nv, 2).copy(), slot=s))
            out[name] = rows
        return out

    def close(self):
        if self._handle:
            self._lib.moog_engine_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # pylint: disable=broad-except
            pass


class SubBatchedEnvironment(object):
    """N envs stepped as G independent sub-batches, each on its own HIP stream (an EnvPool-style surface):

        env = SubBatchedEnvironment(num_envs=4096, sub_batches=4, **config)
        env.reset()
        for g in range(env.sub_batches): env.step_async(g, actions_g)      # returns at once
        ts_g = env.recv(g)                                                 # TimeStep views of sub-batch g

    A `step()` of the whole batch lasts as long as its slowest env (contact-heavy envs take 2.5-3 x the mean,
    DESIGN 3.1), and the next call cannot start before it: the machine idles behind that barrier.  Sub-batches are
    chained only with themselves -- step -> frames -> next step on the sub-batch's stream -- so one sub-batch's slow
    tail runs beside another's head, and frames of one beside steps of another, by plain stream concurrency.

    Results do not depend on G: the parts are ordinary engine handles over contiguous slices of ONE set of tensors
    (`state_f64`, `image`, ... are whole-batch tensors here), and the random streams are keyed by the global env
    index, so env i computes exactly what it computes in a BatchedEnvironment of num_envs.

    Stream contract: `step_async(g, a)` makes sub-batch g's stream wait for the work already queued on the caller's
    current stream (the producer of `a`); `recv(g)` makes the caller's current stream wait for sub-batch g.  A consumer
    that wants the overlap must not funnel every sub-batch through one stream between recv and step_async: use
    `stream(g)` (e.g. `with torch.cuda.stream(env.stream(g))`) for the per-sub-batch policy work, or queue several
    steps ahead.  `step(actions)` / `reset()` are the synchronous whole-batch forms."""

    def __init__(self, state_initializer, physics, task, action_space, observers, game_rules=(),
                 meta_state_initializer=None, num_envs=1, sub_batches=2, device=None, seed=0, env_index0=0,
                 layer_capacity=None, keep_sprite_factors=False, reset_pool='auto', action_repeat=1):
        import torch
        self._torch = torch
        if layer_capacity == 'auto' or (isinstance(layer_capacity, dict) and layer_capacity.get('auto')):
            # (growing a layer re-creates the engine over new records: the sub-batches are views of ONE set of tensors)
            raise NotImplementedError("SubBatchedEnvironment: layer_capacity='auto' is not available; pass {layer: slots} "
                                      "(BatchedEnvironment(layer_capacity='auto').layer_usage() reports the demand)")
        if meta_state_initializer is not None or any(getattr(r, 'host_side', False) for r in game_rules):
            raise NotImplementedError('SubBatchedEnvironment: host-side meta-state rules step the whole batch on the host')
        G = int(sub_batches)
        if G < 1 or num_envs % G != 0:
            raise ValueError('num_envs (%d) must be a multiple of sub_batches (%d)' % (num_envs, G))
        self.num_envs, self.sub_batches = int(num_envs), G
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.compiled = _compiler.compile_config(
            state_initializer, physics, task, action_space, observers, game_rules, None,
            layer_capacity=layer_capacity, keep_sprite_factors=keep_sprite_factors)
        P, L = self.compiled.program, self.compiled.layout
        self.layout = L
        with torch.cuda.device(self.device):
            bufs = BatchedEnvironment.allocate_buffers(torch, L, P, self.num_envs, self.device)
            self._streams = [torch.cuda.Stream(device=self.device) for _ in range(G)]
            self.view_images = BatchedEnvironment.allocate_view_buffers(torch, self.compiled, self.num_envs, self.device)
            self.tables = BatchedEnvironment.allocate_table_buffers(torch, self.compiled, self.num_envs, self.device)
        (self.state_f64, self.state_i32, self.reward, self.discount, self.step_type, self.image) = bufs
        with torch.cuda.device(self.device):   # (BatchedEnvironment.repeat_count, whole batch: every part writes its slice)
            self.repeat_count = torch.zeros((self.num_envs,), dtype=torch.int32, device=self.device)
        m = self.num_envs // G
        self.part_envs = m
        self.parts = []
        for g in range(G):
            part = slice(g * m, (g + 1) * m)
            views = PartBuffers(*(b[part] for b in bufs), view_images={k: t[part] for k, t in self.view_images.items()},
                                repeat_count=self.repeat_count[part], tables={k: t[part] for k, t in self.tables.items()})
            self.parts.append(BatchedEnvironment(
                state_initializer, physics, task, action_space, observers, game_rules, None,
                num_envs=m, device=self.device, seed=seed, env_index0=int(env_index0) + g * m,
                reset_pool=reset_pool, action_repeat=action_repeat, _compiled=self.compiled, _buffers=views))
        self.physics, self.task, self.action_space = physics, task, action_space
        self.observers, self.game_rules = observers, game_rules
        self._is_grid = self.parts[0]._is_grid
        self._pending = [None] * G   # per sub-batch: the event of its last queued call

    def stream(self, g):
        return self._streams[g]

    @property
    def action_repeat(self):
        return self.parts[0].action_repeat

    def set_action_repeat(self, k):
        """BatchedEnvironment.set_action_repeat for every sub-batch (from each one's next queued call on)."""
        for p in self.parts:
            p._check_action_repeat(k)
        for p in self.parts:
            p.set_action_repeat(k)

    def part_slice(self, g):
        return slice(g * self.part_envs, (g + 1) * self.part_envs)

    def enable_cost_schedule(self, enabled=True):
        """Cost-ordered launch inside every sub-batch (BatchedEnvironment.enable_cost_schedule)."""
        for g, p in enumerate(self.parts):
            with self._torch.cuda.stream(self._streams[g]):
                p.enable_cost_schedule(enabled)

    def _enqueue(self, g, fn):
        torch = self._torch
        s = self._streams[g]
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            out = fn()
            ev = torch.cuda.Event()
            ev.record(s)
        self._pending[g] = ev
        return out

    def step_async(self, g, action):
        """Queues one step of sub-batch g (actions [num_envs / G, ...]) on its stream and returns."""
        if hasattr(action, 'record_stream') and action.is_cuda:
            action.record_stream(self._streams[g])
        self._enqueue(g, lambda: self.parts[g].step(action))

    def reset_async(self, g):
        self._enqueue(g, lambda: self.parts[g].reset())

    def recv(self, g):
        """TimeStep of sub-batch g's last queued call (views of the whole-batch tensors); the caller's current stream
        waits for it."""
        if self._pending[g] is not None:
            self._torch.cuda.current_stream(self.device).wait_event(self._pending[g])
        return self.parts[g]._timestep()

    def _join(self):
        cur = self._torch.cuda.current_stream(self.device)
        for ev in self._pending:
            if ev is not None:
                cur.wait_event(ev)

    def _timestep(self):
        from .observers import raw_state
        obs = {}
        for key, o in self.observers.items():   # every observer, in the config's order (as BatchedEnvironment._observation)
            if isinstance(o, raw_state.RawState):
                obs[key] = raw_state.StateView(self)
            elif key == self.compiled.observer_key:
                obs[key] = self.image
            elif key in self.tables:
                obs[key] = self.tables[key]
            else:
                obs[key] = self.view_images[key]
        return dm_env.TimeStep(self.step_type, self.reward, self.discount, obs)

    def reset(self):
        for g in range(self.sub_batches):
            self.reset_async(g)
        self._join()
        return self._timestep()

    def step(self, action):
        """Whole-batch synchronous form: every sub-batch steps, the caller's stream waits for all of them."""
        m = self.part_envs
        for g in range(self.sub_batches):
            self.step_async(g, action[g * m:(g + 1) * m])
        self._join()
        return self._timestep()

    def rollout(self, actions, record=None):
        """BatchedEnvironment.rollout of the whole batch, synchronous: the actions are packed once, every sub-batch runs its
        [T, num_envs / G, ...] slice of them on its own stream and writes its slice of one [T, num_envs] reward tensor (no
        copies: the engine takes the strides), the caller's stream waits for all of them.  Returns (timestep, rewards,
        repeat_count) of the whole batch; the results do not depend on G.  record: as BatchedEnvironment.rollout -- one
        [T, num_envs, rows, columns] tensor per key, sub-batch g recording into [:, g m:(g + 1) m] of it."""
        torch = self._torch
        p0 = self.parts[0]
        keys = None if record is None else p0._check_record(record)
        T = p0._check_rollout(p0._sequence_length(actions))
        a = p0._pack_sequence(actions, self.num_envs)
        with torch.cuda.device(self.device):
            rewards = torch.empty((T, self.num_envs), dtype=torch.float64, device=self.device)
        traj = None if keys is None else p0._new_trajectory(keys, T, self.num_envs)
        m = self.part_envs
        for g in range(self.sub_batches):
            a.record_stream(self._streams[g])
            rewards.record_stream(self._streams[g])
            part = None
            if traj is not None:
                for t in traj.values():
                    t.record_stream(self._streams[g])
                part = {key: t[:, g * m:(g + 1) * m] for key, t in traj.items()}
            self._enqueue(g, lambda g=g, part=part: self.parts[g]._rollout_packed(
                a[:, g * m:(g + 1) * m], rewards[:, g * m:(g + 1) * m], part))
        self._join()
        if traj is None:
            return self._timestep(), rewards, self.repeat_count
        return self._timestep(), rewards, self.repeat_count, traj

    def rollout_candidates(self, actions, record=None):
        """BatchedEnvironment.rollout_candidates of the whole batch, synchronous: the actions are packed once, sub-batch g
        evaluates its [:, :, g m:(g + 1) m] slice of them on its own stream and writes its slices of the whole-batch
        outputs (no copies: the engine takes the strides), the caller's stream waits for all of them.  The results do not
        depend on G, and no sub-batch's state changes."""
        p0 = self.parts[0]
        keys = None if record is None else p0._check_record(record)
        K, T = p0._check_candidates(*p0._candidate_dims(actions))
        a = p0._pack_candidates(actions, self.num_envs)
        rewards, count, ended, traj = p0._new_candidate_outputs(K, T, keys, self.num_envs)
        m = self.part_envs
        for g in range(self.sub_batches):
            for t in [a, rewards, count, ended] + list((traj or {}).values()):
                t.record_stream(self._streams[g])
            part = None if traj is None else {key: t[:, :, g * m:(g + 1) * m] for key, t in traj.items()}
            self._enqueue(g, lambda g=g, part=part: self.parts[g]._rollout_candidates_packed(
                a[:, :, g * m:(g + 1) * m], rewards[:, :, g * m:(g + 1) * m], count[:, g * m:(g + 1) * m],
                ended[:, g * m:(g + 1) * m], part))
        self._join()
        return (rewards, count, ended) if traj is None else (rewards, count, ended, traj)

    def random_action(self):
        torch = self._torch
        if self._is_grid:
            return torch.randint(0, 5, (self.num_envs,), dtype=torch.int32, device=self.device)
        return torch.rand((self.num_envs, 2), dtype=torch.float64, device=self.device) * 2 - 1

    def observation_spec(self):
        return self.parts[0].observation_spec()

    def action_spec(self):
        return self.parts[0].action_spec()

    def raise_faults(self):
        self._torch.cuda.synchronize(self.device)
        for p in self.parts:
            p.raise_faults()

    def set_timing(self, enabled, kernels=None, every=1):
        for p in self.parts:
            p.set_timing(enabled, kernels, every)

    def kernel_time(self, kernel_id):
        """(total ms, launches) summed over the sub-batches' engines."""
        ms, cnt = 0.0, 0
        for p in self.parts:
            a, b = p.kernel_time(kernel_id)
            ms += a
            cnt += b
        return ms, cnt

    def field(self, name):
        return BatchedEnvironment.field(self, name)

    def table_rows(self, key):
        return self.parts[0].table_rows(key)

    def segmentation_rows(self, key):
        return self.parts[0].segmentation_rows(key)

    def ray_rows(self, key):
        return self.parts[0].ray_rows(key)

    def contact_rows(self, key):
        return self.parts[0].contact_rows(key)

    def ray_directions(self, key):
        return self.parts[0].ray_directions(key)

    def table_columns(self, key):
        return self.parts[0].table_columns(key)

    def sprites(self, env=0):
        return BatchedEnvironment.sprites(self, env)

    def close(self):
        self._torch.cuda.synchronize(self.device)
        for p in self.parts:
            p.close()


class Environment(object):
    """Single-env facade with the reference's dm_env semantics (environment.py:28-158):
    numpy observation, Python-scalar reward, `None` reward/discount on FIRST."""

    def __init__(self, state_initializer, physics, task, action_space, observers, game_rules=(),
                 meta_state_initializer=None, **engine_kwargs):
        self._batched = BatchedEnvironment(
            state_initializer, physics, task, action_space, observers, game_rules,
            meta_state_initializer, num_envs=1, **engine_kwargs)
        self.physics = physics
        self.task = task
        self.action_space = action_space
        self.observers = observers
        self.game_rules = game_rules
        self.step_count = 0

    def _unbatch(self, ts):
        st = dm_env.StepType(int(ts.step_type[0].item()))
        obs = self._host_obs(ts.observation)
        self.step_count = int(self._batched.step_count[0].item())
        if st == dm_env.StepType.FIRST:
            return dm_env.TimeStep(st, None, None, obs)
        return dm_env.TimeStep(st, float(ts.reward[0].item()), float(ts.discount[0].item()), obs)

    def reset(self):
        return self._unbatch(self._batched.reset())

    def step(self, action):
        if isinstance(action, dict):   # Composite: {key: sub-action}
            keys = self._batched.action_space.action_keys
            packed = np.zeros((1, len(keys), 2))
            for i, key in enumerate(keys):
                v = np.asarray(action[key], dtype=np.float64).reshape(-1)
                packed[0, i, :len(v)] = v
            return self._unbatch(self._batched.step(packed))
        a = np.asarray(action)
        if self._batched._is_grid:
            a = a.reshape(1)
        else:
            a = a.reshape(1, 2).astype(np.float64)
        return self._unbatch(self._batched.step(a))

    @staticmethod
    def _host_obs(observation):
        """numpy frame; a RawState entry becomes the env's OrderedDict of sprite dicts
        (observers/raw_state.py:17-19 passes the state itself)."""
        return {k: (v.sprites(0) if hasattr(v, 'sprites') else v[0].cpu().numpy())
                for k, v in observation.items()}

    def observation(self):
        return self._host_obs(self._batched.observation())

    def observation_spec(self):
        return self._batched.observation_spec()

    def action_spec(self):
        return self._batched.action_spec()

    @property
    def reset_next_step(self):
        return bool(self._batched.reset_next_step[0].item())

    @property
    def meta_state(self):
        return self._batched.meta_state

    @property
    def batched(self):
        return self._batched

    def close(self):
        self._batched.close()
