// moog_engine.hip -- kernels and C ABI of the MI355X batched MOOG step engine.
//
// Kernels (all gfx950, wave64):
//   moog_reset_kernel   one wavefront per env; device-side state initialisation
//                       (rejection sampler) for masked / auto-resetting envs
//   moog_step_kernel    one wavefront per env; rules -> action -> K physics
//                       substeps -> task, state record staged in LDS
//   moog_raster_kernel  one 256-thread workgroup per env; PIL-exact scanline
//                       polygon fill, painter's order composed in registers,
//                       coalesced 16-byte stores of the uint8 frame
// The C ABI at the bottom is what include/moog_engine.h declares.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "moog_kernels.h"

#include "moog_raster.h"
#include "moog_sprite_table.h"
#include "moog_ray_sensor.h"
#include "moog_contacts.h"
#include <dlfcn.h>
#include <unistd.h>

// =====================================================================================
// host side: engine object + C ABI
// =====================================================================================
static thread_local std::string g_err;
static const char* const FRAMELESS_MSG = "this program draws no frames (no PILRenderer observer: render 0 x 0): pass no image";
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(x)                                                                        \
  do {                                                                                   \
    hipError_t err_ = (x);                                                               \
    if (err_ != hipSuccess)                                                              \
      return fail(MOOG_E_HIP, std::string(#x) + ": " + hipGetErrorString(err_));         \
  } while (0)

struct TimedKernel {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  double total_ms = 0;
  int64_t launches = 0;
  int64_t seq = 0;   // launches seen while timing is on (every `period`-th one is bracketed)
};

// Everything the engine holds per render configuration: views[0] draws the program's `render` (the primary: the config's first
// PILRenderer), views[1 ..] the extra renderers of moog_engine_add_view.  Shared between views, in moog_engine: the static
// prefix's scratch record (s_f64 / s_i32: a reset does not depend on the renderer), the anti-aliasing scratch canvas (launches
// on a stream are serial) and the per-env prefix (the primary's only).
struct RView {
  moog_render_t render{};
  const moog_program_t* P = nullptr;   // the device program the span kernel reads `render` from: the engine's for the primary,
  moog_program_t* d_own = nullptr;     // for an extra view a copy of it with `render` replaced (d_own)
  uint8_t* image = nullptr;            // an extra view's bound frames (moog_engine_set_view_image), or null
  RPlan raster_plan_{};
  RmSetup mask_setup{};   // the mask rasteriser (moog_raster_mask_core.h): ok = this view's ordinary frames are drawn by it
  uint8_t* draw = nullptr;        // its input: a draw record per env (moog_draw_record.h), written by the step kernel or derived before the launch
  RmDrawLayout draw_lay{};
  int raster_tile_w = 0, raster_band_h = 0, raster_tiles_x = 1, raster_bands = 1;   // one workgroup per tile of the canvas
  // anti_aliasing > 1: frames are drawn on a canvas aa x the observation (a chunk of envs at a time) and down-sampled
  int aa = 1, canvas_w = 0, canvas_h = 0, aa_chunk = 0;
  int pad_w = 0;                  // canvas_w rounded up to a multiple of 16: the width the rasteriser draws (pil_renderer.py:64-66
                                  // accepts any size; the extra columns are what Pillow would draw on a wider image, and are dropped)
  uint8_t* pad_img = nullptr;     // [n_envs][canvas_h][pad_w][3] when pad_w != canvas_w without anti-aliasing (cropped into the caller's frames)
  int32_t* aa_tables = nullptr;   // bounds + coefficients of both axes
  RResize aa_resize{};
  int raster_chunk = 0, raster_words = 0, raster_iwords = 0, raster_hwords = 1, raster_xxcap = 4;
  size_t raster_lds = 0;
  int32_t* rows_seen = nullptr;    // two pinned host words: the most polygon rows a frame wanted when that was more than the mask rasteriser's row records; how many frames did
  int raster_rows_fixed = 0;       // MOOG_RASTER_ROWS pins the records (tests of the multi-pass path)
  int mask_free_cap = 0;           // the most row records that cost no resident frame per CU (mask_free_rows)
  // static prefix of the rasteriser (moog_raster.h): the reference sprites (moog_engine::s_f64 / s_i32) and their picture
  int n_static = 0, nsv = 0, kept_n_static = 0;   // (kept: while a colour override has the prefix switched off)
  uint8_t* s_bg = nullptr;
};

// An observer of the engine that a launch of its own refreshes (launch_tables): a sprite table (moog_engine_add_table), a ray
// sensor (moog_engine_add_sensor) or a contacts observer (moog_engine_add_contacts).  Each is the kernel's descriptor, the device
// arrays the descriptor points into (its rows; a sensor's directions too), and -- in desc.out -- the bound buffer
// (moog_engine_set_*_buffer), or null.
template <class Desc>
struct Attached {
  Desc desc{};
  void* d_mem[2] = {nullptr, nullptr};
};
// The observers of one kind: the first n slots are in use (an add call hands out the next), n_bound of them have a buffer.
template <class SlotT, int MAX_>
struct ObserverSet {
  typedef SlotT Slot;
  static constexpr int MAX = MAX_;
  Slot at[MAX_];
  int n = 0, n_bound = 0;
};

// A sprite table has more.  `traj`: what the step kernel's recorder needs of the table (its rows, its column ids) and -- in
// traj.out -- the trajectory bound for the sequences to come (moog_engine_set_table_trajectory).
struct STable : Attached<StTable> {
  TrajTable traj{};
};

// A segmentation of the engine (moog_engine_add_segmentation): the raster state of a view of its size and modifier (always on
// the mask path, no cached prefix), the ids its emitter puts where a view's emitter puts colours, and the bound image, or null.
struct SegView {
  RView v;
  uint32_t* d_ids = nullptr;   // [n_envs][slots] the emitter's rgb_override: slot_id in the low byte (replicated per env: the emitter indexes it by env)
  uint8_t* ids = nullptr;      // [n_envs][height][width] (moog_engine_set_segmentation_image)
  uint8_t* pad_ids = nullptr;  // [n_envs][height][pad_w] when the width is no multiple of 16 (cropped into `ids`)
};

struct moog_engine {
  moog_program_t prog;
  moog_layout_t L;
  moog_program_t* d_prog = nullptr;
  int16_t* d_vslot = nullptr;
  uint32_t* d_vinfo = nullptr;   // rasteriser: vertex slot -> sprite slot | index within the sprite << 8
  int32_t n_envs = 0;
  int device = 0;
  uint64_t seed = 0;
  int64_t env_index0 = 0;
  moog_state_view_t view{nullptr, nullptr};
  size_t step_lds = 0;
  int step_wps = 4;   // register-allocation variant of the step kernel (waves per SIMD)
  void* spec_handle = nullptr;   // a step kernel compiled for this very program (load_spec_kernel), or null
  void (*spec_launch)(int, size_t, hipStream_t, const KArgs*) = nullptr;
  int32_t xstack_off = 0;
  // candidate rollouts (moog_engine_plan_sequences): the LDS of one wavefront with the WHOLE record staged (hot_layout_uncut)
  // and the expression stacks' place in it; a candidate kernel compiled for this very program (load_spec_plan_kernel), or null
  size_t plan_lds = 0;
  int32_t plan_xstack_off = 0;
  void* spec_plan_handle = nullptr;
  void (*spec_plan_launch)(int, size_t, hipStream_t, const KArgs*) = nullptr;
  FOp* d_fops = nullptr;       // flattened force list (moog_flatten_forces)
  int32_t n_fops = 0;
  int32_t* watch = nullptr;     // section sampling (MOOG_WATCH=1): [n_envs][MOOG_WATCH_SECTIONS]
  int32_t watch_off = 0;
  bool dynamic_rules = false;
  bool maze_kernel = false;   // the program uses MazePhysics / a maze walk / a per-reset maze
  bool late_reset = false;    // ... but only to build an episode: it is stepped by the kernels without the rare components, and
                              // the full reset kernel behind every step launch opens the episodes those could not (step_env)
  uint8_t* late_mask = nullptr;   // [n_envs]
  RView views[MOOG_MAX_VIEWS];
  int n_views = 1;               // views[0] and the extra views added so far
  ObserverSet<STable, MOOG_MAX_TABLES> tables;
  ObserverSet<Attached<RsSensor>, MOOG_MAX_SENSORS> sensors;
  ObserverSet<Attached<CtObs>, MOOG_MAX_CONTACTS> contacts;
  SegView segs[MOOG_MAX_SEGMENTATIONS];
  int n_segs = 0, n_bound_segs = 0;       // segmentations added so far; how many of them have an image
  bool frameless = false;        // render 0 x 0: the program draws no frames (no raster state at all)
  uint8_t* aa_canvas = nullptr;   // shared by the anti-aliased views: [aa_chunk][canvas_h][pad_w][3] of whichever is drawn
  uint8_t* aa_tmp = nullptr;      // [aa_chunk][canvas_h][width rounded up to 4][3]
  size_t aa_canvas_bytes = 0, aa_tmp_bytes = 0;
  int timing = 0;   // bit k: launches of kernel k are bracketed by HIP events
  int32_t* perm = nullptr;
  hipStream_t sched_stream = nullptr;   // the launch-order sort runs beside the rasteriser
  hipEvent_t ev_step_done = nullptr, ev_sched_done = nullptr;
  bool sched_pending = false;
  float* cost = nullptr;
  // moog_engine_set_reset_pool: the next episode of every env is built beside the step kernels (moog_kernels.h "reset pool")
  static constexpr int POOL_STREAMS = 8;
  int pool_streams = 2;   // the ones in use: hardware queues the runtime has (GPU_MAX_HW_QUEUES, default 4) minus the caller's and the sort's
  bool pool_on = false, pool_ready = false;
  static constexpr int pool_depth = 2;   // records per env: the next episode and the one after (an episode shorter than a fill does not stall its call)
  int32_t* pool_state = nullptr;   // [pool_depth][n_envs] 0 empty / 3 claimed / 1 being filled / 2 ready
  int32_t* pool_tag = nullptr;     // [pool_depth][n_envs] episode of the pool record
  int32_t* pool_lock = nullptr;    // [n_envs] 4 while the step kernel opens an episode of the env
  unsigned long long* pool_stats = nullptr;   // [4] KArgs::pool_stats
  double* pool_f64[2] = {nullptr, nullptr};   // [pool_depth][n_envs][f64_per_env]: the fill's inputs, the record after its reset
  int32_t* pool_i32[2] = {nullptr, nullptr};
  hipStream_t pool_stream[POOL_STREAMS] = {};   // fills run here, call k's on stream k % pool_streams
  hipEvent_t ev_pool = nullptr;    // the call a fill follows
  int64_t pool_fills = 0;          // fill launches so far
  int act_f32 = 0;               // moog_engine_set_action_dtype: the action buffer holds float32 values
  int action_repeat = 1;         // moog_engine_set_action_repeat: env-steps per call of moog_engine_step
  int32_t* repeat_count = nullptr;   // [n_envs] the env-steps each env took in the call (caller-owned, or null)
  int32_t* layer_hw = nullptr;   // [2 * MOOG_MAX_LAYERS]: high-water mark / dropped appends of the dynamic layers
  TimedKernel timed[MOOG_K_COUNT];
  int32_t* fault_flag = nullptr;   // pinned host word the kernels OR fault bits into
  int step_dbg = 0, raster_stop = 0;   // profiling aids (MOOG_STEP_DEBUG / MOOG_RASTER_STOP at create, moog_engine_set_debug)
  // static prefix of the rasteriser (moog_raster.h): a scratch env record that holds the reference
  // sprites (what a reset makes of the constant generation ops) and their picture
  double* s_f64 = nullptr;
  int32_t* s_i32 = nullptr;
  const uint32_t* rgb_override = nullptr;   // moog_engine_set_color_override
  int kept_pe_ns = 0, kept_pe_nsv = 0;   // the prefixes' sizes while a colour override has them switched off
  // per-env prefix (RArgs::sbg_env_stride): leading sprites that stay put within an episode but differ between envs
  int pe_ns = 0, pe_nsv = 0;        // slots / vertex slots of the prefix (0: off); shrinks to the slots that really stay put
  double* pe_f64 = nullptr;         // [n_envs] snapshot of the record each env's picture was drawn from
  int32_t* pe_i32 = nullptr;
  uint8_t* pe_bg = nullptr;         // [n_envs][canvas_h][pad_w][3]
  int32_t* pe_valid = nullptr;      // [n_envs] the env has a picture
  int32_t* pe_build = nullptr;      // [n_envs] this call's build launch draws the env's picture
  int32_t* pe_min = nullptr;        // pinned host word: first slot of the prefix seen changing in the middle of an episode
};

// ---- what the sprite tables, ray sensors and contacts observers share ----------------------------------------------------------
// The three kinds differ in their describe function (moog_st_describe, moog_rs_describe, moog_ct_describe: descriptor layouts
// and id conventions of their own), in the arrays they upload and in the alignment their kernel's stores need; the rest of an
// add call, a set-buffer call, a launch's gathering and the destroy is here, over ObserverSet.

// An add call's checks; `slot`: where the new observer goes.  It counts only once the call has succeeded (`set.n++`), so a
// call that fails leaves the slot as it found it.
template <class Set>
static int next_observer(moog_engine* e, Set moog_engine::*which, const void* desc, const int32_t* index, const char* full,
                         typename Set::Slot** slot) {
  if (!e || !desc || !index) return fail(MOOG_E_INVALID, "null argument");
  Set& set = e->*which;
  if (set.n >= Set::MAX) return fail(MOOG_E_INVALID, full);
  *slot = &set.at[set.n];
  return MOOG_OK;
}

// Device copies of an observer's arrays (at most two, d_mem of its slot).  A failure frees everything this call allocated.
struct Upload {
  const void* host;
  size_t bytes;
};
static int upload_observer(moog_engine* e, const Upload* up, int n_up, void** d_mem) {
  HIPCHK(hipSetDevice(e->device));
  hipError_t err = hipSuccess;
  for (int k = 0; k < n_up && err == hipSuccess; ++k) {
    err = hipMalloc(&d_mem[k], up[k].bytes);
    if (err == hipSuccess) err = hipMemcpy(d_mem[k], up[k].host, up[k].bytes, hipMemcpyHostToDevice);
  }
  if (err == hipSuccess) return MOOG_OK;
  for (int k = 0; k < n_up; ++k) {
    if (d_mem[k]) hipFree(d_mem[k]);
    d_mem[k] = nullptr;
  }
  (void)hipGetLastError();
  return fail(MOOG_E_HIP, std::string("hipMalloc / hipMemcpy of an observer's arrays: ") + hipGetErrorString(err));
}

// A set-buffer call: binds `dev` (null: unbinds) and keeps the bound count.  align_mask: the address bits that must be 0,
// given the descriptor.
template <class Set>
static int bind_observer(moog_engine* e, Set moog_engine::*which, int32_t index, void* dev, const char* none,
                         uintptr_t (*align_mask)(const decltype(Set::Slot::desc)&), const char* misaligned) {
  if (!e) return fail(MOOG_E_INVALID, "null engine");
  Set& set = e->*which;
  if (index < 0 || index >= set.n) return fail(MOOG_E_INVALID, none);
  auto& d = set.at[index].desc;
  if ((uintptr_t)dev & align_mask(d)) return fail(MOOG_E_INVALID, misaligned);
  set.n_bound += (dev ? 1 : 0) - (d.out ? 1 : 0);
  d.out = (decltype(d.out))dev;
  return MOOG_OK;
}

// The descriptors of a set's bound observers, in index order, into a launch's argument array; how many.
template <class Set, class Desc>
static int gather_bound(const Set& set, Desc* out) {
  int n = 0;
  for (int k = 0; k < set.n; ++k)
    if (set.at[k].desc.out) out[n++] = set.at[k].desc;
  return n;
}

template <class Set>
static void free_observers(Set& set) {
  for (typename Set::Slot& t : set.at)
    for (void* p : t.d_mem)
      if (p) hipFree(p);
}

static void free_engine(moog_engine* e) {
  if (e->d_prog) hipFree(e->d_prog);
  if (e->d_vslot) hipFree(e->d_vslot);
  if (e->d_vinfo) hipFree(e->d_vinfo);
  for (RView& v : e->views) {
    if (v.d_own) hipFree(v.d_own);
    if (v.draw) hipFree(v.draw);
    if (v.s_bg) hipFree(v.s_bg);
    if (v.pad_img) hipFree(v.pad_img);
    if (v.aa_tables) hipFree(v.aa_tables);
    if (v.rows_seen) hipHostFree(v.rows_seen);
  }
  free_observers(e->tables);
  free_observers(e->sensors);
  free_observers(e->contacts);
  for (SegView& g : e->segs) {
    if (g.v.draw) hipFree(g.v.draw);
    if (g.v.rows_seen) hipHostFree(g.v.rows_seen);
    if (g.d_ids) hipFree(g.d_ids);
    if (g.pad_ids) hipFree(g.pad_ids);
  }
  if (e->s_f64) hipFree(e->s_f64);
  if (e->s_i32) hipFree(e->s_i32);
  if (e->aa_canvas) hipFree(e->aa_canvas);
  if (e->aa_tmp) hipFree(e->aa_tmp);
  if (e->fault_flag) hipHostFree(e->fault_flag);
  if (e->layer_hw) hipFree(e->layer_hw);
  for (int k = 0; k < moog_engine::POOL_STREAMS; ++k)
    if (e->pool_stream[k]) { hipStreamSynchronize(e->pool_stream[k]); hipStreamDestroy(e->pool_stream[k]); }
  if (e->ev_pool) hipEventDestroy(e->ev_pool);
  if (e->pe_f64) hipFree(e->pe_f64);
  if (e->pe_i32) hipFree(e->pe_i32);
  if (e->pe_bg) hipFree(e->pe_bg);
  if (e->pe_valid) hipFree(e->pe_valid);
  if (e->pe_build) hipFree(e->pe_build);
  if (e->pe_min) hipHostFree(e->pe_min);
  if (e->pool_state) hipFree(e->pool_state);
  if (e->pool_tag) hipFree(e->pool_tag);
  if (e->pool_lock) hipFree(e->pool_lock);
  if (e->late_mask) hipFree(e->late_mask);
  if (e->pool_stats) hipFree(e->pool_stats);
  for (int k = 0; k < 2; ++k) { if (e->pool_f64[k]) hipFree(e->pool_f64[k]); if (e->pool_i32[k]) hipFree(e->pool_i32[k]); }
  if (e->watch) hipFree(e->watch);
  if (e->d_fops) hipFree(e->d_fops);
  delete e;
}

// Leading sprite slots that every reset creates identically and at rest: slots filled by generation
// ops without a random factor, zero velocity.  Whether a frame's prefix really equals the reference
// is checked by the raster kernel per frame, so this only has to be a good guess.
static int static_prefix_slots(const moog_program_t* p, int polymod, int* nsv) {
  *nsv = 0;
  if (polymod != MOOG_POLYMOD_NONE) return 0;
  std::vector<char> ok((size_t)(p->n_slots > 0 ? p->n_slots : 1), 0);
  for (int oi = 0; oi < p->n_ops; ++oi) {
    const moog_genop_t& op = p->ops[oi];
    if (op.runtime || op.n_sampled != 0 || op.code_off >= 0 || op.count_min != op.count_max) continue;
    bool c = true;
    for (int k = 0; k < MOOG_NUM_FACTORS; ++k) c = c && op.factors[k].kind == MOOG_DIST_CONST;
    c = c && op.factors[MOOG_FAC_XVEL].a == 0 && op.factors[MOOG_FAC_YVEL].a == 0 && op.factors[MOOG_FAC_ANGVEL].a == 0;
    if (!c) continue;
    for (int sl = op.slot0; sl < op.slot0 + op.count_max && sl < p->n_slots; ++sl)
      if (sl >= 0 && !p->layer_dynamic[p->slot_layer[sl]]) ok[sl] = 1;
  }
  int ns = 0, nv = 0;
  while (ns < p->n_slots && ns < 32 && ok[ns] && p->slot_voff[ns] == nv) { nv += p->slot_vcap[ns]; ++ns; }
  *nsv = nv;
  return ns;
}

// Per-env prefix: leading slots whose sprites are created at rest by the initializer (whatever their positions: a maze's
// walls, food on its cells) and that no op's code writes to afterwards.  A guess like the one above: the check launch
// compares every frame's prefix with the env's snapshot, and slots that turn out to change within episodes (food that gets
// eaten) shorten the prefix (launch_raster).
static int env_prefix_slots(const moog_program_t* p, int* nsv) {
  *nsv = 0;
  if (p->render.polymod != MOOG_POLYMOD_NONE) return 0;
  std::vector<char> ok((size_t)(p->n_slots > 0 ? p->n_slots : 1), 0);
  for (int oi = 0; oi < p->n_ops; ++oi) {
    const moog_genop_t& op = p->ops[oi];
    if (op.runtime || op.cell_sel == MOOG_CELL_STORE) continue;
    bool c = true;
    for (int k = MOOG_FAC_XVEL; k <= MOOG_FAC_ANGVEL; ++k)
      if (k == MOOG_FAC_XVEL || k == MOOG_FAC_YVEL || k == MOOG_FAC_ANGVEL) c = c && op.factors[k].kind == MOOG_DIST_CONST && op.factors[k].a == 0;
    if (!c) continue;
    for (int sl = op.slot0; sl < op.slot0 + op.count_max && sl < p->n_slots; ++sl)
      if (sl >= 0 && !p->layer_dynamic[p->slot_layer[sl]]) ok[sl] = 1;
  }
  for (int oi = 0; oi < p->n_ops; ++oi)
    if (p->ops[oi].cell_sel == MOOG_CELL_STORE && p->ops[oi].cell_arg >= 0 && p->ops[oi].cell_arg < p->n_slots) ok[p->ops[oi].cell_arg] = 0;
  int ns = 0, nv = 0;
  while (ns < p->n_slots && ok[ns] && p->slot_voff[ns] == nv) { nv += p->slot_vcap[ns]; ++ns; }
  *nsv = nv;
  return ns;
}

// Which step kernel a program takes, from the program alone (no device): the variant (plain / + expression evaluator,
// run-time sampler, dynamic layers / + the rare components), whether its episodes are opened by the reset kernel behind the
// step kernel (late reset), the LDS of one env and the register-allocation variant that follows from it.  Used by
// moog_engine_create and, through moog_program_step_kernel, by the builder of program-specialised kernels (moog/_spec.py).
struct StepVariant { bool dynamic_rules = false, maze_kernel = false, late_reset = false; int wps = 4; size_t step_lds = 0; int32_t xstack_off = 0;
                     size_t plan_lds = 0; int32_t plan_xstack_off = 0; };   // (plan_*: the candidate kernels', the whole record staged)

static StepVariant step_variant_of(const moog_program_t* prog) {
  StepVariant v;
  moog_layout_t GL;
  moog_layout(prog, &GL);
  const moog_layout_t HL = hot_layout(GL).L;   // the records as staged in LDS
  v.step_lds = (size_t)HL.f64_per_env * 8 + (size_t)HL.i32_per_env * 4 + (size_t)GL.S * 4 * 8 +
               (size_t)((GL.S + 3) & ~3) * 4 + CAND_CAP * 2 + 128 + 64 * 8 + 16;
  if (prog->xstack_depth > 0) {   // per-lane value stacks of the lane-parallel filter evaluator (moog_device.h eval_expr_t<true>)
    v.step_lds = (v.step_lds + 15) & ~(size_t)15;
    v.xstack_off = (int32_t)v.step_lds;
    v.step_lds += (size_t)prog->xstack_depth * 64 * 8;
  }
  // the same areas behind the uncut record (hot_layout_uncut: 3 S doubles and 3 S words more where the step kernels cut them)
  v.plan_lds = (size_t)GL.f64_per_env * 8 + (size_t)GL.i32_per_env * 4 + (size_t)GL.S * 4 * 8 +
               (size_t)((GL.S + 3) & ~3) * 4 + CAND_CAP * 2 + 128 + 64 * 8 + 16;
  if (prog->xstack_depth > 0) {
    v.plan_lds = (v.plan_lds + 15) & ~(size_t)15;
    v.plan_xstack_off = (int32_t)v.plan_lds;
    v.plan_lds += (size_t)prog->xstack_depth * 64 * 8;
  }
  for (int r = 0; r < prog->n_rules; ++r) {
    int k = prog->rules[r].kind;
    if (k == MOOG_RULE_VANISH_BY_FILTER || k == MOOG_RULE_CHANGE_LAYER || k == MOOG_RULE_CREATE_SPRITES ||
        k == MOOG_RULE_MODIFY_SPRITES || k == MOOG_RULE_MODIFY_ON_CONTACT || k == MOOG_RULE_DRAWS)
      v.dynamic_rules = true;
  }
  for (int t = 0; t < prog->n_tasks; ++t) {
    if (prog->tasks[t].kind == MOOG_TASK_CONTACT_REWARD && (prog->tasks[t].xcond >= 0 || prog->tasks[t].xreward >= 0))
      v.dynamic_rules = true;
    if (prog->tasks[t].kind == MOOG_TASK_RESET && (prog->tasks[t].cond >= MOOG_COND_ALL_EXPR || prog->tasks[t].xreward >= 0))
      v.dynamic_rules = true;   // (a reward_fn that reads the state is an expression too: task_reward<DYN> evaluates it)
  }
  for (int r = 0; r < prog->n_rules; ++r)
    if ((prog->rules[r].kind == MOOG_RULE_CONDITIONAL || prog->rules[r].kind == MOOG_RULE_PHASE) &&
        prog->rules[r].cond >= MOOG_RCOND_CONTACT_COUNT)
      v.dynamic_rules = true;   // (rule_gate is compiled into both variants; keep them together anyway)
  for (int l = 0; l < prog->n_layers; ++l) if (prog->layer_dynamic[l]) v.dynamic_rules = true;
  for (int f = 0; f < prog->n_forces; ++f)   // a traced force_fn runs in the expression evaluator
    if (prog->forces[f].kind == MOOG_FORCE_DISTANCE_EXPR) v.dynamic_rules = true;
  for (int r = 0; r < prog->n_rules; ++r)
    if (prog->rules[r].kind == MOOG_RULE_FIXATION || (prog->rules[r].kind == MOOG_RULE_PHASE && prog->rules[r].op == 1))
      v.dynamic_rules = true;
  for (int k = 0; k < prog->n_dcode; ++k) {   // assigning sprite.angle turns the path: in the kernels that carry every component
    if (prog->dcode[k].op == MOOG_X_STORE && prog->dcode[k].a == MOOG_XA_ANGLE) v.maze_kernel = true;
    // expressions that name sprites by slot (state-level task functions: Reset(condition / reward_fn), and the reset-time
    // code) use opcodes only those kernels' evaluator carries (moog_device.h eval_expr_t: MOOG_WITH_MAZE)
    const int op = prog->dcode[k].op;
    if (op == MOOG_X_SLOT_ATTR || op == MOOG_X_HDRAW || op == MOOG_X_HDRAW_T || op == MOOG_X_STORE_VERT || op == MOOG_X_FACTOR)
      v.maze_kernel = true;
  }
  for (int o = 0; o < prog->n_ops; ++o) if (prog->ops[o].cell_sel != MOOG_CELL_NONE) v.maze_kernel = true;   // maze / draw / shuffle ops
  if (prog->n_hdraws > 0) v.maze_kernel = true;   // reset-time expressions: in the kernels that carry every component (m3 / m4)
  for (int o = 0; o < prog->n_ops; ++o)
    for (int k = 0; k < MOOG_NUM_FACTORS; ++k)
      if (prog->ops[o].factors[k].kind == MOOG_DIST_EXPR || prog->ops[o].factors[k].kind == MOOG_DIST_EXPR_SHAPE)
        v.maze_kernel = true;
  // the maze components live in a kernel variant of their own (m3 / m4): their code would only enlarge the others
  for (int f = 0; f < prog->n_forces; ++f)
    if (prog->forces[f].kind == MOOG_FORCE_MAZE_WALK || prog->forces[f].kind == MOOG_FORCE_MAZE_WALK_DET) v.maze_kernel = true;
  for (int c = 0; c < prog->n_corrective; ++c) if (prog->corrective[c].kind == MOOG_CORR_MAZE) v.maze_kernel = true;
  if (prog->maze.random) v.maze_kernel = true;
  if (v.maze_kernel) {
    // What the program needs WHILE STEPPING of the components only the every-component kernels carry: maze walks and
    // MazePhysics, modifiers that assign sprite.angle, run-time generators with maze cells / computed factors.  Everything else
    // that selects those kernels (reset-time draws and expressions, maze generation, shuffles, choices, look-aheads, values an
    // initializer keeps across episodes) happens when an episode is built.
    bool stepping = false;
    for (int f = 0; f < prog->n_forces; ++f)
      stepping = stepping || prog->forces[f].kind == MOOG_FORCE_MAZE_WALK || prog->forces[f].kind == MOOG_FORCE_MAZE_WALK_DET;
    for (int c = 0; c < prog->n_corrective; ++c) stepping = stepping || prog->corrective[c].kind == MOOG_CORR_MAZE;
    for (int k = 0; k < prog->n_dcode; ++k) stepping = stepping || (prog->dcode[k].op == MOOG_X_STORE && prog->dcode[k].a == MOOG_XA_ANGLE);
    for (int o = 0; o < prog->n_ops; ++o) {
      const moog_genop_t& op = prog->ops[o];
      if (!op.runtime) continue;
      bool full = op.cell_sel != MOOG_CELL_NONE || op.code_off >= 0;
      for (int k = 0; k < MOOG_NUM_FACTORS; ++k)
        full = full || op.factors[k].kind == MOOG_DIST_EXPR || op.factors[k].kind == MOOG_DIST_EXPR_SHAPE;
      stepping = stepping || full;
    }
    const char* off = getenv("MOOG_NO_LATE_RESET");
    v.late_reset = !stepping && !(off && atoi(off));
    if (v.late_reset) v.dynamic_rules = true;   // (the variant with the expression evaluator)
  }
  // register allocation: three waves per SIMD (168 VGPRs) when the LDS of an env allows no more than 14 envs per CU anyway
  v.wps = (160 * 1024 / (v.step_lds ? v.step_lds : 1)) <= 14 ? 3 : 4;
  { const char* w = getenv("MOOG_STEP_WPS"); if (w && (atoi(w) == 3 || atoi(w) == 4)) v.wps = atoi(w); }   // experiments, tests
  return v;
}

static uint64_t program_hash(const moog_program_t* prog) {   // FNV-1a 64 over the program's bytes (moog/_spec.py computes the same)
  const unsigned char* b = reinterpret_cast<const unsigned char*>(prog);
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < sizeof(moog_program_t); ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

// A step kernel compiled for exactly this program (csrc/moog_step_spec.hip), if one has been built: looked for as
// <MOOG_SPEC_DIR or the directory of this library + "/spec">/step_<hash>_d<variant>w<wps>.so.  Everything about it is
// checked -- the digest of the kernel sources and flags it was built from, ABI, argument struct, variant, and the embedded
// program byte for byte -- before it replaces the generic kernel.
static void load_spec_kernel(moog_engine* e, const moog_program_t* prog);
// ... and the candidate kernel compiled for it, plan_<hash>_d<variant>w<wps>.so beside that object, checked the same way
static void load_spec_plan_kernel(moog_engine* e, const moog_program_t* prog);

// The digest of the kernel sources and flags this library was built from (moog/_digest.py; -DMOOG_SRC_DIGEST=0x...ull on the
// command line of this unit and of every program-specialised step kernel).  0: built without one -- no specialised kernel loads.
#ifndef MOOG_SRC_DIGEST
#define MOOG_SRC_DIGEST 0ull
#endif
#define MOOG_STR2(x) #x
#define MOOG_STR(x) MOOG_STR2(x)
extern "C" const char moog_src_digest_marker[] = "MOOG_SRC_DIGEST=" MOOG_STR(MOOG_SRC_DIGEST);   // (read as text by moog/_digest.py)

extern "C" {

int moog_abi_version(void) { return MOOG_ABI_VERSION; }
unsigned long long moog_source_digest(void) { return MOOG_SRC_DIGEST; }
const char* moog_last_error(void) { return g_err.c_str(); }
int64_t moog_program_sizeof(void) { return (int64_t)sizeof(moog_program_t); }

static int validate_render(const moog_program_t* p, const moog_render_t* r) {
  const int aa = r->aa > 1 ? r->aa : 1;
  const long long cw = (long long)aa * r->width, ch = (long long)aa * r->height;
  if (cw < 1 || cw > 8192 || ch < 1 || ch > 8192 || aa > 16)
    return fail(MOOG_E_UNSUPPORTED, "render size unsupported (1 <= anti_aliasing x width, height <= 8192, anti_aliasing <= 16)");
  if (r->cmap != MOOG_CMAP_IDENTITY && r->cmap != MOOG_CMAP_HSV) return fail(MOOG_E_INVALID, "render cmap out of range");
  if (r->polymod != MOOG_POLYMOD_NONE && r->polymod != MOOG_POLYMOD_TORUS && r->polymod != MOOG_POLYMOD_FIRST_PERSON)
    return fail(MOOG_E_INVALID, "render polymod out of range");
  if (r->polymod == MOOG_POLYMOD_FIRST_PERSON && (r->polymod_layer < 0 || r->polymod_layer >= p->n_layers))
    return fail(MOOG_E_INVALID, "render polymod_layer out of range");
  return MOOG_OK;
}

static int validate(const moog_program_t* p) {
  if (!p) return fail(MOOG_E_INVALID, "null program");
  if (p->abi_version != MOOG_PROGRAM_VERSION) return fail(MOOG_E_INVALID, "program abi_version mismatch");
  if (p->n_slots < 0 || p->n_slots > MOOG_MAX_SLOTS) return fail(MOOG_E_INVALID, "n_slots out of range");
  if (p->n_layers < 0 || p->n_layers > MOOG_MAX_LAYERS) return fail(MOOG_E_INVALID, "n_layers out of range");
  if (p->n_hdraws < 0 || p->n_hdraws > MOOG_MAX_HDRAWS) return fail(MOOG_E_INVALID, "n_hdraws out of range");
  if (p->updates_per_env_step < 1) return fail(MOOG_E_INVALID, "updates_per_env_step < 1");
  for (int s = 0; s < p->n_slots; ++s)
    if (p->slot_vcap[s] > 128) return fail(MOOG_E_UNSUPPORTED, "sprites with more than 128 vertices");
  // the pairwise forces (collisions, gravity, springs) scan a layer pair's candidates 64 / 128 at a time
  for (int f = 0; f < p->n_forces; ++f) {
    const moog_force_t* F = &p->forces[f];
    if (F->n_b <= 0) continue;
    for (int k = 0; k < F->n_a; ++k)
      if (p->layer_nslots[F->layers_a[k]] > 64 * 2) return fail(MOOG_E_UNSUPPORTED, "layer of a pairwise force too large");
    for (int k = 0; k < F->n_b; ++k)
      if (p->layer_nslots[F->layers_b[k]] > 64 * 2) return fail(MOOG_E_UNSUPPORTED, "layer of a pairwise force too large");
  }
  if (p->maze.random && (p->maze.gen_size < 1 || p->maze.gen_size > MOOG_MAX_MAZE_GEN || p->maze.size < p->maze.gen_size ||
                         p->maze.size > MOOG_MAX_MAZE))
    return fail(MOOG_E_UNSUPPORTED, "random maze size unsupported");
  if (!(p->render.width == 0 && p->render.height == 0)) {   // (0 x 0: the program draws no frames)
    const int rc = validate_render(p, &p->render);
    if (rc) return rc;
  }
  return MOOG_OK;
}

static KArgs make_args(moog_engine* e, const void* actions, const moog_inject_t* inj,
                       const moog_step_out_t* out, int mode, const uint8_t* mask);
static RArgs raster_args(moog_engine* e, RView& v, uint8_t* image);

// Pillow Resample.c precompute_coeffs + normalize_coeffs_8bpc for the LANCZOS filter (support 3): the window of
// output sample xx is centred on (xx + 0.5) * scale, weights are normalised in double and rounded to fixed
// point with 22 fractional bits.  Returns the taps per output sample.
static int resize_coeffs(int in_size, int out_size, std::vector<int32_t>& bounds, std::vector<int32_t>& kk) {
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 3.0 * filterscale;
  const int ksize = (int)std::ceil(support) * 2 + 1;
  auto sinc = [](double x) { return x == 0.0 ? 1.0 : std::sin(x * M_PI) / (x * M_PI); };
  auto lanczos = [&](double x) { return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3) : 0.0; };
  bounds.assign(2 * (size_t)out_size, 0);
  kk.assign((size_t)out_size * ksize, 0);
  std::vector<double> pre((size_t)ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = 0 + (xx + 0.5) * scale, ss = 1.0 / filterscale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    int x;
    for (x = 0; x < xmax; ++x) {
      const double w = lanczos((x + xmin - center + 0.5) * ss);
      pre[x] = w;
      ww += w;
    }
    for (x = 0; x < xmax; ++x)
      if (ww != 0.0) pre[x] /= ww;
    for (; x < ksize; ++x) pre[x] = 0;
    for (x = 0; x < ksize; ++x)
      kk[(size_t)xx * ksize + x] = pre[x] < 0 ? (int)(-0.5 + pre[x] * (1 << 22)) : (int)(0.5 + pre[x] * (1 << 22));
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  return ksize;
}

static int setup_anti_aliasing(moog_engine* e, RView& v) {
  if (v.aa <= 1) return MOOG_OK;
  const int ow = v.render.width, oh = v.render.height;
  std::vector<int32_t> bh, bv, ch, cv;
  const int kh = resize_coeffs(v.canvas_w, ow, bh, ch), kv = resize_coeffs(v.canvas_h, oh, bv, cv);
  const size_t words = bh.size() + bv.size() + ch.size() + cv.size();
  if (hipMalloc(&v.aa_tables, words * sizeof(int32_t)) != hipSuccess) return fail(MOOG_E_NOMEM, "hipMalloc(resize tables) failed");
  int32_t* d = v.aa_tables;
  HIPCHK(hipMemcpy(d, bh.data(), bh.size() * 4, hipMemcpyHostToDevice)); const int32_t* dbh = d; d += bh.size();
  HIPCHK(hipMemcpy(d, bv.data(), bv.size() * 4, hipMemcpyHostToDevice)); const int32_t* dbv = d; d += bv.size();
  HIPCHK(hipMemcpy(d, ch.data(), ch.size() * 4, hipMemcpyHostToDevice)); const int32_t* dch = d; d += ch.size();
  HIPCHK(hipMemcpy(d, cv.data(), cv.size() * 4, hipMemcpyHostToDevice)); const int32_t* dcv = d;
  int hspan = 0;   // the horizontal pass stages the bytes a block of 256 output columns reads in LDS
  for (int x0 = 0; x0 < ow; x0 += 256) {
    const int xl = (x0 + 255 < ow ? x0 + 255 : ow - 1);
    const int b0 = 3 * bh[2 * x0] & ~3, b1 = 3 * (bh[2 * xl] + bh[2 * xl + 1]);
    if (b1 - b0 > hspan) hspan = b1 - b0;
  }
  hspan = (hspan + 7) & ~3;
  const int tstride = (ow + 3) & ~3;
  v.aa_resize = RResize{v.canvas_w, v.canvas_h, ow, oh, kh, kv, dbh, dbv, dch, dcv, hspan, v.pad_w, tstride};
  // canvases of a chunk of envs at a time: at most 1 GiB of scratch, one scratch for every view (launches on a stream are
  // serial): it grows to the largest view's
  const size_t canvas = (size_t)v.pad_w * v.canvas_h * 3;
  size_t chunk = ((size_t)1 << 30) / canvas;
  if (chunk < 1) chunk = 1;
  if (chunk > (size_t)e->n_envs) chunk = (size_t)e->n_envs;
  v.aa_chunk = (int)chunk;
  const size_t cb = chunk * canvas, tb = chunk * (size_t)v.canvas_h * tstride * 3;
  if (cb > e->aa_canvas_bytes || tb > e->aa_tmp_bytes) {
    if (e->aa_canvas || e->aa_tmp) HIPCHK(hipDeviceSynchronize());   // (an earlier call's launches may still use the old scratch)
    if (cb > e->aa_canvas_bytes) {
      if (e->aa_canvas) hipFree(e->aa_canvas);
      e->aa_canvas = nullptr; e->aa_canvas_bytes = 0;
      if (hipMalloc(&e->aa_canvas, cb) != hipSuccess) return fail(MOOG_E_NOMEM, "hipMalloc(anti-aliasing canvas) failed");
      e->aa_canvas_bytes = cb;
    }
    if (tb > e->aa_tmp_bytes) {
      if (e->aa_tmp) hipFree(e->aa_tmp);
      e->aa_tmp = nullptr; e->aa_tmp_bytes = 0;
      if (hipMalloc(&e->aa_tmp, tb) != hipSuccess) return fail(MOOG_E_NOMEM, "hipMalloc(anti-aliasing canvas) failed");
      e->aa_tmp_bytes = tb;
    }
  }
  return MOOG_OK;
}

// Resets one scratch env (the constant generation ops do not depend on the random stream) and renders
// its static prefix on top of the background colour: the reference record and picture of moog_raster.h.
// The scratch record is the same for every view (a reset does not depend on the renderer): made once, by the first view
// that has a prefix; each view draws its own picture from it.
static int build_static_prefix(moog_engine* e, RView& v) {
  int nsv = 0;
  const int ns = getenv("MOOG_RASTER_NO_STATIC") ? 0 : static_prefix_slots(&e->prog, v.render.polymod, &nsv);
  if (ns == 0) return MOOG_OK;
  const size_t pb = (size_t)v.pad_w * v.canvas_h * 3;
  if (hipMalloc(&v.s_bg, pb) != hipSuccess) return fail(MOOG_E_NOMEM, "hipMalloc(static prefix) failed");
  const moog_state_view_t keep = e->view;
  const int32_t keep_n = e->n_envs;
  if (!e->s_f64) {
    const size_t fb = (size_t)e->L.f64_per_env * 8, ib = (size_t)e->L.i32_per_env * 4;
    if (hipMalloc(&e->s_f64, fb) != hipSuccess || hipMalloc(&e->s_i32, ib) != hipSuccess)
      return fail(MOOG_E_NOMEM, "hipMalloc(static prefix) failed");
    HIPCHK(hipMemset(e->s_f64, 0, fb));
    HIPCHK(hipMemset(e->s_i32, 0, ib));
    e->view.f64 = e->s_f64; e->view.i32 = e->s_i32; e->n_envs = 1;
    KArgs a = make_args(e, nullptr, nullptr, nullptr, MODE_RESET_MASK, nullptr);
    a.dbg = 0;
    a.fault_flag = nullptr;   // (faults of the scratch env are nobody's business)
    (e->maze_kernel ? moog_launch_reset_full : moog_launch_reset_plain)(1, e->step_lds, 0, a);
  }
  e->view.f64 = e->s_f64; e->view.i32 = e->s_i32; e->n_envs = 1;
  RArgs r = raster_args(e, v, v.s_bg);
  r.n_static = ns; r.nsv = nsv; r.build = 1; r.debug_stop = 0;
  moog_raster_launch(r, v.raster_lds, 0);
  e->view = keep; e->n_envs = keep_n;
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(0));
  v.n_static = ns; v.nsv = nsv;
  return MOOG_OK;
}

// Per-env prefix (RArgs::sbg_env_stride): worth its memory (a frame and a record per env) and its two extra launches per
// call when it covers many sprites of a frame that takes several workgroups -- measured (profiles/r04_env_prefix.txt):
// pacman's 256 x 256 frames (136 walls, 8 tiles) 2.51 -> 1.73 ms per 4096; one-tile frames (maze_zoo, functional_maze)
// lose 0.09 ms to the check and the build launch and gain nothing, their workgroups being bound by fixed costs.
// MOOG_RASTER_ENV_BG=0 turns it off, =1 turns it on whatever the frame size (A/B runs, tests).
// The mask rasteriser's row records per pass (moog_raster_mask_core.h): `cap` of them, at least a canvas height so that any one
// polygon fits, at most one per (polygon, canvas row) and 4096 (the row sort's 12-bit places), and no more than 64 KB of LDS
// leave room for.  ok = 0 when even the smallest plan does not fit.
static void mask_plan_rows(moog_engine* e, RView& v, int cap) {
  RmSetup& ms = v.mask_setup;
  if (cap > 4096) cap = 4096;
  if (cap > ms.S * v.canvas_h) cap = ms.S * v.canvas_h;
  if (cap < v.canvas_h) cap = v.canvas_h;
  for (;;) {
    rm_plan(ms.S, e->L.TOTV * ms.ncopy, v.pad_w, v.canvas_h, cap, ms.iwords, RM_THREADS / 64, ms.big, &ms.plan, ms.compact);
    if (ms.plan.total <= 64u * 1024u || cap <= v.canvas_h) break;
    cap = cap - 64 > v.canvas_h ? cap - 64 : v.canvas_h;
  }
  ms.cap_rows = cap;
  ms.lds = ms.plan.total;
  if (ms.plan.total > 64u * 1024u) ms.ok = 0;
}

// A frame with more polygon rows than row records is drawn in several passes, each a full sweep over the frame: correct, and
// cheaper than it sounds -- what costs is a resident frame less per CU (profiles/r05_raster.txt 5: cleanup's raster launch takes 97 us
// with 192 or 384 records and 1390 us with the 1500 its busiest frames would like).  So frames that want more records say so
// through a host-mapped word and before a later launch the records grow AS FAR AS THAT IS FREE: the same number of frames per
// CU (LDS; registers hold ten, and a plan within 1 KB of losing one counts as losing it).  falling_balls_64's launch 628 -> 471 us.
// They never shrink; the picture does not depend on their number.  Once they are as many as is free the frames stop reporting
// (an atomic on host memory per frame and launch: 8.6 ms per launch when every frame of a batch of 4096 keeps doing it).
static int mask_frames_per_cu(uint32_t lds) {   // by LDS, and by registers: RM_WAVES_PER_SIMD waves on each of four SIMDs, RM_THREADS / 64 waves a frame
  const int n = (int)(160u * 1024u / (lds + 1024u)), by_regs = RM_WAVES_PER_SIMD * 4 / (RM_THREADS / 64);
  return n > by_regs ? by_regs : n;
}
// the most row records that cost no resident frame per CU against the plan in hand (called once, at create)
static int mask_free_rows(moog_engine* e, RView& v) {
  RmSetup& ms = v.mask_setup;
  const RmSetup first = ms;
  int best = first.cap_rows;
  for (int cap = first.cap_rows + 32; cap <= 4096; cap += 32) {
    ms = first;
    mask_plan_rows(e, v, cap);
    if (!ms.ok || ms.cap_rows < cap || mask_frames_per_cu(ms.lds) < mask_frames_per_cu(first.lds)) break;
    best = cap;
  }
  ms = first;
  return best;
}
static void mask_rows_grow(moog_engine* e, RView& v) {
  if (!v.rows_seen || v.raster_rows_fixed || v.mask_setup.cap_rows >= v.mask_free_cap) return;
  const int want = __atomic_load_n(&v.rows_seen[0], __ATOMIC_RELAXED);
  RmSetup& ms = v.mask_setup;
  if (want <= ms.cap_rows) return;
  const RmSetup before = ms;
  int cap = (want + want / 8 + 31) & ~31;
  if (cap > v.mask_free_cap) cap = v.mask_free_cap;
  mask_plan_rows(e, v, cap);
  if (!ms.ok || ms.cap_rows <= before.cap_rows) ms = before;
}

static int setup_env_prefix(moog_engine* e) {
  const RView& v = e->views[0];
  const char* sw = getenv("MOOG_RASTER_ENV_BG");
  if ((sw && atoi(sw) == 0) || v.aa > 1) return MOOG_OK;
  const bool forced = sw && atoi(sw) == 1;
  int nsv = 0;
  const int ns = env_prefix_slots(&e->prog, &nsv);
  const size_t frame = (size_t)v.canvas_h * v.pad_w * 3;
  if (ns < 16 || ns < v.n_static + 8 || (size_t)e->n_envs * frame > ((size_t)4 << 30)) return MOOG_OK;
  if (!forced && (v.raster_tiles_x * v.raster_bands < 2 || ns < 32)) return MOOG_OK;
  const size_t n = (size_t)e->n_envs;
  if (hipMalloc(&e->pe_f64, n * e->L.f64_per_env * 8) != hipSuccess || hipMalloc(&e->pe_i32, n * e->L.i32_per_env * 4) != hipSuccess ||
      hipMalloc(&e->pe_bg, n * frame) != hipSuccess || hipMalloc(&e->pe_valid, n * 4) != hipSuccess ||
      hipMalloc(&e->pe_build, n * 4) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&e->pe_min), sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
    (void)hipGetLastError();   // no room: the frames are drawn without it
    return MOOG_OK;
  }
  HIPCHK(hipMemset(e->pe_valid, 0, n * 4));
  *e->pe_min = INT32_MAX;
  e->pe_ns = ns; e->pe_nsv = nsv;
  return MOOG_OK;
}

// The raster state of one view (a render configuration over this engine's program): canvas and tile geometry, the span
// kernel's LDS plan, the mask rasteriser's setup and its draw records.  The per-env prefix is the primary's only.
static int setup_view(moog_engine* e, RView& v, bool primary) {
  const moog_program_t* prog = &e->prog;
  // raster LDS plan (moog_raster.h): row records for `chunk` rows per pass
  {
    // Tiles: the row masks of the kernel are 128 bits, so a wider canvas is cut into columns of the widest
    // multiple of 16 <= 128 that divides the width, and a taller one into bands of 64 rows.
    v.aa = v.render.aa > 1 ? v.render.aa : 1;
    v.canvas_w = v.aa * v.render.width;
    v.canvas_h = v.aa * v.render.height;
    v.pad_w = (v.canvas_w + 15) & ~15;
    int tw = v.pad_w <= 128 ? v.pad_w : 128;
    while (v.pad_w % tw != 0) tw -= 16;
    v.raster_tile_w = tw;
    v.raster_tiles_x = v.pad_w / tw;
    v.raster_band_h = v.canvas_h <= 128 ? v.canvas_h : 64;
    {   // (the primary's only: extra views never use the per-env prefix)
        // frames that will use the per-env prefix (setup_env_prefix): few sprites are left to draw per tile and the per-tile fixed
        // cost dominates -- whole-height tiles measured 1.65 against 1.73 ms per 4096 pacman frames (profiles/r04_env_prefix.txt)
        // (decided here, from what the PROGRAM allows: the tile plan sizes every LDS table.  A handle that later runs without the prefix --
        //  allocation failure, a prefix that shrank to nothing, a colour override -- keeps the whole-height tiles: 1.65 ms against 1.73 ms
        //  with 64-row bands WITH the prefix, 2.45 against 2.51 ms WITHOUT it in the same file: not a loss either way)
      int nsv_ = 0;
      const char* sw = getenv("MOOG_RASTER_ENV_BG");
      if (primary && v.canvas_h > 128 && v.canvas_h <= 256 && v.aa <= 1 && !(sw && atoi(sw) == 0) && env_prefix_slots(prog, &nsv_) >= 32)
        v.raster_band_h = v.canvas_h;
    }
    v.raster_bands = (v.canvas_h + v.raster_band_h - 1) / v.raster_band_h;
    int W = v.raster_tile_w, H = v.raster_band_h;   // (the LDS plan is per tile)
    int ncopy = v.render.polymod == MOOG_POLYMOD_TORUS ? 9 : 1;
    int items = prog->n_slots * ncopy;
    if (items < 1) items = 1;
    v.raster_words = (W + 63) / 64;
    v.raster_iwords = (items + 31) / 32;
    int maxv = 2;
    for (int sl = 0; sl < prog->n_slots; ++sl) if (prog->slot_vcap[sl] > maxv) maxv = prog->slot_vcap[sl];
    v.raster_xxcap = 2 * maxv;
    v.raster_hwords = (maxv + 31) / 32;
    RPlan pl;
    // Row records per pass: 376 (>= H so that any item fits; sized so that six workgroups of the
    // 4096 x 32-sprite workload share a CU), then as many more as fit without costing a resident
    // workgroup (frames with more rows than records take several passes).
    int cap = items * H;
    if (cap > 376) cap = 376;
    if (cap < H) cap = H;
    raster_plan(prog->n_slots, e->L.TOTV, ncopy, W, H, cap, v.raster_iwords, v.raster_hwords, v.raster_xxcap, &pl);
    {
      const unsigned lds_cu = 160 * 1024;
      unsigned wgs = pl.total ? lds_cu / pl.total : 0;
      if (wgs > 6) wgs = 6;   // registers hold six workgroups per CU at most
      const int want = items * H < 4096 ? items * H : 4096;
      while (wgs && cap < want) {
        RPlan p2;
        int c2 = cap + 32 < want ? cap + 32 : want;
        raster_plan(prog->n_slots, e->L.TOTV, ncopy, W, H, c2, v.raster_iwords, v.raster_hwords, v.raster_xxcap, &p2);
        if (lds_cu / p2.total < wgs) break;
        cap = c2; pl = p2;
      }
    }
    { const char* rc = getenv("MOOG_RASTER_ROWS"); if (rc && atoi(rc) >= H) cap = atoi(rc); }   // tuning / tests of the multi-pass path
    raster_plan(prog->n_slots, e->L.TOTV, ncopy, W, H, cap, v.raster_iwords, v.raster_hwords, v.raster_xxcap, &pl);
    if (pl.total > 160 * 1024 || (size_t)e->L.TOTV * ncopy >= (1u << 20)) {
      return fail(MOOG_E_UNSUPPORTED, "raster working set does not fit in LDS");
    }
    v.raster_chunk = cap;
    v.raster_plan_ = pl;
    v.raster_lds = pl.total;
  }
  {   // mask rasteriser (moog_raster_mask_core.h): one-tile frames, polygons of <= 128 vertices, at most 256 polygons (a torus has nine per sprite)
    RmSetup& ms = v.mask_setup;
    memset(&ms, 0, sizeof ms);
    int maxv = 1;
    for (int sl = 0; sl < prog->n_slots; ++sl) if (prog->slot_vcap[sl] > maxv) maxv = prog->slot_vcap[sl];
    const int ncopy = v.render.polymod == MOOG_POLYMOD_TORUS ? 9 : 1;
    const char* sw = getenv("MOOG_RASTER_MASK");   // 0: the push / sort / span kernel for every frame (A/B runs, tests)
    ms.ok = !(sw && atoi(sw) == 0) && v.raster_tiles_x * v.raster_bands == 1 && v.pad_w <= 128 && v.canvas_h <= 128 &&
            maxv <= RM_BIG_NV && prog->n_slots >= 1 && prog->n_slots * ncopy <= 256 && e->L.TOTV >= 1;
    if (ms.ok) {
      ms.slots = prog->n_slots; ms.ncopy = ncopy; ms.big = maxv > RM_MAX_NV ? 1 : 0;
      ms.S = prog->n_slots * ncopy;
      ms.iwords = (ms.S + 31) / 32;
      ms.cmap = v.render.cmap;
      ms.first_person = v.render.polymod == MOOG_POLYMOD_FIRST_PERSON ? 1 : 0;
      if (ms.first_person) { ms.fp_slot0 = prog->layer_slot0[v.render.polymod_layer]; ms.fp_nslots = prog->layer_nslots[v.render.polymod_layer]; }
      ms.bg = ((uint32_t)v.render.bg[0] & 255u) | (((uint32_t)v.render.bg[1] & 255u) << 8) | (((uint32_t)v.render.bg[2] & 255u) << 16);
      // row records per pass: 192 (the headline workload's frames have ~170 rows behind the cached walls), at least a
      // canvas height so that any one polygon fits; frames with more rows take several passes
      // (frames that want more keep the records growing: mask_rows_grow, before a launch)
      int cap = 192;
      { const char* rc = getenv("MOOG_RASTER_ROWS"); if (rc && atoi(rc) >= 1) { cap = atoi(rc); v.raster_rows_fixed = 1; } }   // tuning / tests of the multi-pass path
      mask_plan_rows(e, v, cap);
      {   // 4-byte edge records when the 16-byte ones keep frames off a CU (or do not fit at all): MOOG_RASTER_COMPACT=0 / 1 forces
        const char* cs = getenv("MOOG_RASTER_COMPACT");
        const RmSetup full = ms;
        ms.compact = 1; ms.ok = 1;
        mask_plan_rows(e, v, cap);
        // (the 4-byte records cost the rows phase a tenth more instructions -- headline workload 49.5 -> 53 us when they were picked for
        //  it by mistake -- so they are for programs whose 16-byte records leave a CU clearly short of the frames its registers allow)
        const int by_regs = RM_WAVES_PER_SIMD * 4 / (RM_THREADS / 64);
        const bool better = ms.ok && (!full.ok || ((int)(160u * 1024u / full.lds) < by_regs - 1 && mask_frames_per_cu(ms.lds) > mask_frames_per_cu(full.lds)));
        if (cs ? atoi(cs) == 0 : !better) ms = full;
      }
      v.mask_free_cap = (ms.ok && !v.raster_rows_fixed) ? mask_free_rows(e, v) : ms.cap_rows;
      if (ms.ok) {   // a draw record per env (moog_draw_record.h): header + an item per slot and copy + every vertex slot's point and owner byte
        v.draw_lay = rm_draw_layout(ms.S, e->L.TOTV * ms.ncopy);
        if (hipMalloc(&v.draw, (size_t)e->n_envs * v.draw_lay.stride) != hipSuccess) {
          return fail(MOOG_E_NOMEM, "out of device memory (draw records)");
        }
      }
    }
  }
  // (coherent = fine-grained: the kernels' system-scope atomics and the host's atomic read / clear meet in the same memory)
  if (hipHostMalloc(reinterpret_cast<void**>(&v.rows_seen), 2 * sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) { v.rows_seen[0] = 0; v.rows_seen[1] = 0; }   // ([1]: how many frames wanted more: for tools)
  else v.rows_seen = nullptr;   // (without it the records keep their first size)
  return MOOG_OK;
}

int moog_engine_create(const moog_program_t* prog, int32_t n_envs, int32_t device_id, uint64_t seed,
                       int64_t env_index0, moog_engine_t** out) {
  if (!out) return fail(MOOG_E_INVALID, "null out");
  int rc = validate(prog);
  if (rc) return rc;
  if (n_envs <= 0) return fail(MOOG_E_INVALID, "n_envs <= 0");
  HIPCHK(hipSetDevice(device_id));
  moog_engine* e = new moog_engine();
  e->prog = *prog;
  e->frameless = prog->render.width == 0 && prog->render.height == 0;
  moog_layout(prog, &e->L);
  e->n_envs = n_envs;
  e->device = device_id;
  e->seed = seed;
  e->env_index0 = env_index0;
  hipError_t err = hipMalloc(&e->d_prog, sizeof(moog_program_t));
  if (err != hipSuccess) { free_engine(e); return fail(MOOG_E_NOMEM, "hipMalloc(program) failed"); }
  err = hipMemcpy(e->d_prog, prog, sizeof(moog_program_t), hipMemcpyHostToDevice);
  if (err != hipSuccess) { free_engine(e); return fail(MOOG_E_HIP, "hipMemcpy(program) failed"); }
  {
    std::vector<int16_t> vs((size_t)(prog->n_total_verts > 0 ? prog->n_total_verts : 1), 0);
    for (int sl = 0; sl < prog->n_slots; ++sl)
      for (int k = 0; k < prog->slot_vcap[sl]; ++k) vs[prog->slot_voff[sl] + k] = (int16_t)sl;
    err = hipMalloc(&e->d_vslot, vs.size() * sizeof(int16_t));
    if (err == hipSuccess)
      err = hipMemcpy(e->d_vslot, vs.data(), vs.size() * sizeof(int16_t), hipMemcpyHostToDevice);
    if (err != hipSuccess) { free_engine(e); return fail(MOOG_E_NOMEM, "vertex table"); }
    std::vector<uint32_t> vi(vs.size(), 0u);
    for (int sl = 0; sl < prog->n_slots; ++sl)
      for (int k = 0; k < prog->slot_vcap[sl]; ++k) vi[prog->slot_voff[sl] + k] = (uint32_t)sl | ((uint32_t)k << 8);
    err = hipMalloc(&e->d_vinfo, vi.size() * sizeof(uint32_t));
    if (err == hipSuccess)
      err = hipMemcpy(e->d_vinfo, vi.data(), vi.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (err != hipSuccess) { free_engine(e); return fail(MOOG_E_NOMEM, "vertex table"); }
  }
  {
    const std::vector<FOp> fops = moog_flatten_forces(prog);
    e->n_fops = (int32_t)fops.size();
    err = hipMalloc(&e->d_fops, (fops.size() + 1) * sizeof(FOp));
    if (err == hipSuccess && !fops.empty()) err = hipMemcpy(e->d_fops, fops.data(), fops.size() * sizeof(FOp), hipMemcpyHostToDevice);
    if (err != hipSuccess) { free_engine(e); return fail(MOOG_E_NOMEM, "force list"); }
  }
  {
    const StepVariant sv = step_variant_of(prog);
    e->step_lds = sv.step_lds; e->xstack_off = sv.xstack_off;
    e->plan_lds = sv.plan_lds; e->plan_xstack_off = sv.plan_xstack_off;
  }
  { const char* w = getenv("MOOG_WATCH");   // section sampling (moog_engine_read_watch): two words of LDS for the watcher
    if (w && atoi(w) == 1) {
      e->step_lds = (e->step_lds + 15) & ~(size_t)15;
      e->watch_off = (int32_t)e->step_lds;
      e->step_lds += 16;
      if (hipMalloc(&e->watch, (size_t)n_envs * MOOG_WATCH_SECTIONS * sizeof(int32_t)) != hipSuccess ||
          hipMemset(e->watch, 0, (size_t)n_envs * MOOG_WATCH_SECTIONS * sizeof(int32_t)) != hipSuccess) {
        free_engine(e);
        return fail(MOOG_E_NOMEM, "hipMalloc(watch) failed");
      }
    } }
  if (e->step_lds > 160 * 1024) {
    free_engine(e);
    return fail(MOOG_E_UNSUPPORTED, "state record does not fit in 160 KB of LDS");
  }
  if (!e->frameless) {
    e->views[0].render = prog->render;
    e->views[0].P = e->d_prog;
    const int rc = setup_view(e, e->views[0], true);
    if (rc) { free_engine(e); return rc; }
  }
  {
    int (*const configure[18])(size_t) = {moog_configure_step_f3, moog_configure_step_f4, moog_configure_step_t3,
                                          moog_configure_step_t4, moog_configure_step_m3, moog_configure_step_m4,
                                          moog_configure_step_f3r, moog_configure_step_f4r, moog_configure_step_t3r,
                                          moog_configure_step_t4r, moog_configure_step_m3r, moog_configure_step_m4r,
                                          moog_configure_step_f3rt, moog_configure_step_f4rt, moog_configure_step_t3rt,
                                          moog_configure_step_t4rt, moog_configure_step_m3rt, moog_configure_step_m4rt};
    for (int v = 0; v < 18 && err == hipSuccess; ++v) err = (hipError_t)configure[v](e->step_lds);
    // the candidate kernels stage the whole record: a record that fits only with its cuts steps, and refuses to plan
    int (*const configure_plan[6])(size_t) = {moog_configure_step_f3rp, moog_configure_step_f4rp, moog_configure_step_t3rp,
                                               moog_configure_step_t4rp, moog_configure_step_m3rp, moog_configure_step_m4rp};
    if (e->plan_lds > 160 * 1024) e->plan_lds = 0;
    for (int v = 0; v < 6 && e->plan_lds && err == hipSuccess; ++v) err = (hipError_t)configure_plan[v](e->plan_lds);
  }
  {
    const StepVariant sv = step_variant_of(prog);
    e->dynamic_rules = sv.dynamic_rules; e->maze_kernel = sv.maze_kernel; e->late_reset = sv.late_reset; e->step_wps = sv.wps;
  }
  if (!e->watch) load_spec_kernel(e, prog);
  if (!e->watch && e->plan_lds) load_spec_plan_kernel(e, prog);
  if (e->late_reset) {
    if (hipMalloc(&e->late_mask, (size_t)n_envs) != hipSuccess || hipMemset(e->late_mask, 0, (size_t)n_envs) != hipSuccess) {
      free_engine(e);
      return fail(MOOG_E_NOMEM, "hipMalloc(late reset mask) failed");
    }
  }
  if (err == hipSuccess)
    err = (hipError_t)moog_configure_reset_plain(e->step_lds);
    if (err == hipSuccess) err = (hipError_t)moog_configure_reset_full(e->step_lds);
  if (err == hipSuccess && !e->frameless)
    err = (hipError_t)moog_raster_configure(e->views[0].raster_lds);
  if (err == hipSuccess && e->views[0].mask_setup.ok) err = (hipError_t)moog_raster_configure_mask(64 * 1024);   // (the records may grow: mask_rows_grow)
  if (err != hipSuccess) {
    free_engine(e);
    return fail(MOOG_E_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(err));
  }
  { const char* ds = getenv("MOOG_STEP_DEBUG"); e->step_dbg = ds ? atoi(ds) : 0; }
  { const char* ds = getenv("MOOG_RASTER_STOP"); e->raster_stop = ds ? atoi(ds) : 0; }
  if (hipHostMalloc(reinterpret_cast<void**>(&e->fault_flag), sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
    free_engine(e);
    return fail(MOOG_E_NOMEM, "hipHostMalloc(fault flag) failed");
  }
  *e->fault_flag = 0;
  for (int l = 0; l < prog->n_layers; ++l)
    if (prog->layer_dynamic[l] && !e->layer_hw) {
      if (hipMalloc(&e->layer_hw, 2 * MOOG_MAX_LAYERS * sizeof(int32_t)) != hipSuccess ||
          hipMemset(e->layer_hw, 0, 2 * MOOG_MAX_LAYERS * sizeof(int32_t)) != hipSuccess) {
        free_engine(e);
        return fail(MOOG_E_NOMEM, "hipMalloc(layer usage) failed");
      }
    }
  int rc2 = MOOG_OK;
  if (!e->frameless) {
    RView& v = e->views[0];
    rc2 = build_static_prefix(e, v);
    if (rc2 == MOOG_OK) rc2 = setup_anti_aliasing(e, v);
    if (rc2 == MOOG_OK) rc2 = setup_env_prefix(e);
    if (rc2 == MOOG_OK && v.aa <= 1 && v.pad_w != v.canvas_w &&
        hipMalloc(&v.pad_img, (size_t)n_envs * v.canvas_h * v.pad_w * 3) != hipSuccess)
      rc2 = fail(MOOG_E_NOMEM, "hipMalloc(16-aligned frames) failed");
  }
  if (rc2) { free_engine(e); return rc2; }
  *out = e;
  return MOOG_OK;
}

static void drain(TimedKernel& t) {
  for (auto& pr : t.pending) {
    hipEventSynchronize(pr.second);
    float ms = 0;
    if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { t.total_ms += ms; t.launches++; }
    hipEventDestroy(pr.first);
    hipEventDestroy(pr.second);
  }
  t.pending.clear();
}

int moog_engine_destroy(moog_engine_t* e) {
  if (!e) return MOOG_OK;
  for (int k = 0; k < MOOG_K_COUNT; ++k) drain(e->timed[k]);
  if (e->sched_stream) {
    hipStreamSynchronize(e->sched_stream);
    hipEventDestroy(e->ev_step_done); hipEventDestroy(e->ev_sched_done);
    hipStreamDestroy(e->sched_stream);
  }
  void* spec = e->spec_handle;
  free_engine(e);
  (void)spec;   // (the object stays mapped: unloading a code object that a stream may still reference is not worth the risk)
  return MOOG_OK;
}

int moog_engine_layout(const moog_engine_t* e, moog_layout_t* out) {
  if (!e || !out) return fail(MOOG_E_INVALID, "null argument");
  *out = e->L;
  return MOOG_OK;
}

static int pool_drop(moog_engine* e, hipStream_t s);

int moog_engine_load_state(moog_engine_t* e, const moog_state_view_t* view) {
  if (!e || !view || !view->f64 || !view->i32) return fail(MOOG_E_INVALID, "null state view");
  if (((uintptr_t)view->f64 & 15) || ((uintptr_t)view->i32 & 15))
    return fail(MOOG_E_INVALID, "state buffers must be 16-byte aligned");
  e->view = *view;
  if (e->pool_on) {   // other records: whatever the pool holds was built from the old ones
    HIPCHK(hipSetDevice(e->device));
    const int rc = pool_drop(e, 0);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(0));
  }
  return MOOG_OK;
}

// (an event pair costs ~5 us of stream time: `period` > 1 samples the launches instead of bracketing all of them)
static bool sampled(moog_engine* e, int id) {
  const int period = ((e->timing >> 8) & 255) + 1;
  return ((e->timing >> id) & 1) && (e->timed[id].seq++ % period) == 0;
}

struct Bracket {
  moog_engine* e; int id; hipStream_t s; hipEvent_t a = nullptr, b = nullptr;
  Bracket(moog_engine* e_, int id_, hipStream_t s_, int on = -1) : e(e_), id(id_), s(s_) {   // on: -1 = sample, else decided
    if (on < 0 ? sampled(e, id) : on != 0) { hipEventCreate(&a); hipEventCreate(&b); hipEventRecord(a, s); }
  }
  ~Bracket() {
    if (a) { hipEventRecord(b, s); e->timed[id].pending.emplace_back(a, b); }
  }
};

static KArgs make_args(moog_engine* e, const void* actions, const moog_inject_t* inj,
                       const moog_step_out_t* out, int mode, const uint8_t* mask) {
  KArgs a;
  a.P = e->d_prog; a.L = e->L; a.H = hot_layout(e->L); a.f64 = e->view.f64; a.i32 = e->view.i32;
  a.actions = actions;
  a.inj = (inj && inj->uniforms) ? inj->uniforms : nullptr;
  a.inj_n = (inj && inj->uniforms) ? inj->per_env : 0;
  a.n_envs = e->n_envs; a.seed = e->seed; a.env_index0 = e->env_index0;
  a.mask = mask;
  a.reward = out ? out->reward : nullptr;
  a.discount = out ? out->discount : nullptr;
  a.step_type = out ? out->step_type : nullptr;
  a.mode = mode;
  a.vslot = e->d_vslot;
  a.perm = (mode == MODE_STEP && e->perm) ? e->perm : nullptr;
  a.cost = (mode == MODE_STEP) ? e->cost : nullptr;
  a.dbg = e->step_dbg;
  a.fault_flag = e->fault_flag;
  a.layer_hw = e->layer_hw;
  a.act_f32 = e->act_f32;
  a.repeat = mode == MODE_STEP ? e->action_repeat : 1;
  a.repeat_count = mode == MODE_STEP ? e->repeat_count : nullptr;
  a.act_step_bytes = 0; a.reward_seq = nullptr; a.reward_seq_stride = 0;   // (moog_engine_step_sequence sets the three)
  memset(a.traj, 0, sizeof a.traj);   // (... and the trajectories bound with moog_engine_set_table_trajectory: no other call records)
  a.n_cand = 0; a.act_cand_bytes = 0; a.reward_cand_stride = 0; a.plan_count = nullptr; a.plan_ended = nullptr;   // (moog_engine_plan_sequences)
  a.count_cand_stride = 0; memset(a.traj_cand_elems, 0, sizeof a.traj_cand_elems);
  a.xstack_off = e->xstack_off;
  a.watch = (mode == MODE_STEP) ? e->watch : nullptr; a.watch_off = e->watch_off;
  a.fops = e->d_fops; a.n_fops = e->n_fops;
  const bool pool = e->pool_on && mode == MODE_STEP && !(inj && inj->uniforms);
  a.pool_state = pool ? e->pool_state : nullptr; a.pool_tag = e->pool_tag; a.pool_stats = e->pool_stats;
  a.pool_lock = e->pool_lock; a.pool_depth = e->pool_depth;
  for (int k = 0; k < 2; ++k) { a.pool_f64[k] = e->pool_f64[k]; a.pool_i32[k] = e->pool_i32[k]; }
  a.live_f64 = nullptr; a.live_i32 = nullptr;
  a.late_mask = (mode == MODE_STEP && e->late_reset) ? e->late_mask : nullptr;
  a.rank0 = 0;
  memset(&a.draw, 0, sizeof a.draw);   // (moog_engine_step turns the draw records on)
  a.draw_vinfo = e->d_vinfo;
  return a;
}

// A specialised kernel carries no profiling word and no section watcher (csrc/moog_kernels.h KDBG): with either set the engine
// steps with the generic kernels, which compute the same results.
static bool steps_specialised(const moog_engine* e) { return e->spec_launch && e->step_dbg == 0 && !e->watch; }

static void launch_step(moog_engine* e, hipStream_t s, const KArgs& a) {
  // (the second six: the kernels with the action-repeat loop, for calls that take more than one env-step and for action
  //  sequences, whose per-step rewards the one-step kernels do not write; the third six: those with the trajectory recorder
  //  as well, for sequences with a trajectory bound -- with a profiling word or a watcher set too: these are generic kernels)
  static const moog_step_launch_fn launch[18] = {moog_launch_step_f3, moog_launch_step_f4, moog_launch_step_t3,
                                                 moog_launch_step_t4, moog_launch_step_m3, moog_launch_step_m4,
                                                 moog_launch_step_f3r, moog_launch_step_f4r, moog_launch_step_t3r,
                                                 moog_launch_step_t4r, moog_launch_step_m3r, moog_launch_step_m4r,
                                                 moog_launch_step_f3rt, moog_launch_step_f4rt, moog_launch_step_t3rt,
                                                 moog_launch_step_t4rt, moog_launch_step_m3rt, moog_launch_step_m4rt};
  if (steps_specialised(e)) {
    e->spec_launch(e->n_envs, e->step_lds, s, &a);
    return;
  }
  const bool full = e->maze_kernel && !e->late_reset;
  launch[(a.traj[0].out ? 12 : (a.repeat > 1 || a.reward_seq) ? 6 : 0) + (full ? 4 : (e->dynamic_rules ? 2 : 0)) + (e->step_wps == 4 ? 1 : 0)](e->n_envs, e->step_lds, s, a);
}

// What the draw-record emitter needs (moog_draw_record.h): by value in the step kernel's and the derive kernel's arguments.
// out = null when this engine's frames are not the mask rasteriser's.
static RmEmit emit_args(moog_engine* e, const RView& v) {
  RmEmit m;
  memset(&m, 0, sizeof m);
  const RmSetup& ms = v.mask_setup;
  if (!ms.ok || !v.draw) return m;
  m.out = v.draw; m.lay = v.draw_lay;
  m.S = ms.S; m.slots = ms.slots; m.ncopy = ms.ncopy; m.W = v.pad_w; m.H = v.canvas_h; m.scale_w = v.canvas_w;
  m.cmap = ms.cmap; m.first_person = ms.first_person; m.fp_slot0 = ms.fp_slot0; m.fp_nslots = ms.fp_nslots;
  m.n_static = (e->s_f64 && ms.ncopy == 1) ? v.n_static : 0;
  m.sref_v = e->s_f64 ? e->s_f64 + e->L.o_verts : nullptr;
  m.sref_col = e->s_f64 ? e->s_f64 + e->L.o_color : nullptr;
  m.sref_flags = e->s_i32 ? e->s_i32 + e->L.o_flags : nullptr;
  m.sref_nv = e->s_i32 ? e->s_i32 + e->L.o_nverts : nullptr;
  m.sref_opa = e->s_i32 ? e->s_i32 + e->L.o_opacity : nullptr;
  m.rgb_override = e->rgb_override;
  return m;
}
// The step kernel writes the draw records of the frames the raster launch behind it draws (moog_engine_step with an image):
// when those frames are the mask rasteriser's, drawn in one launch over every env (a late-reset program's episodes are opened by
// the reset kernel behind the step kernel: that launch writes the draw records of the envs it resets).
static bool step_emits_draw(moog_engine* e) {
  const RView& v = e->views[0];
  // (the emitter's scratch in the step kernel's LDS, emit_draw_record: a torus's nine items per slot must fit behind the vertex offsets)
  const bool scratch_fits = v.mask_setup.ncopy == 1 ||
      4u * (size_t)RM_EMIT_SCRATCH_WORDS(v.mask_setup.slots, v.mask_setup.S, v.mask_setup.ncopy) <= (size_t)CAND_CAP * 2 + 128 + 64 * 8;
  return v.mask_setup.ok && v.draw && e->pe_ns <= 0 && v.aa <= 1 && scratch_fits;
}

static RArgs raster_args(moog_engine* e, RView& v, uint8_t* image) {
  RArgs r;
  if (v.mask_setup.ok) mask_rows_grow(e, v);
  r.ms = v.mask_setup;
  // (frames report only while the records can still grow: every report is an atomic on host memory)
  r.rows_seen = (v.raster_rows_fixed || v.mask_setup.cap_rows >= v.mask_free_cap) ? nullptr : v.rows_seen;
  r.P = v.P; r.L = e->L; r.f64 = e->view.f64; r.i32 = e->view.i32; r.image = image;
  r.vinfo = e->d_vinfo; r.plan = v.raster_plan_;
  r.n_envs = e->n_envs; r.chunk = v.raster_chunk; r.words = v.raster_words;
  r.tile_w = v.raster_tile_w; r.band_h = v.raster_band_h; r.tiles_x = v.raster_tiles_x; r.bands = v.raster_bands;
  r.canvas_w = v.pad_w; r.scale_w = v.canvas_w; r.canvas_h = v.canvas_h; r.flip = v.aa > 1 ? 0 : 1;
  r.iwords = v.raster_iwords; r.hwords = v.raster_hwords; r.xxcap = v.raster_xxcap;
  r.debug_stop = e->raster_stop;
  r.n_static = v.n_static; r.nsv = v.nsv; r.build = 0;
  r.sref_v = e->s_f64 ? e->s_f64 + e->L.o_verts : nullptr;
  r.sref_col = e->s_f64 ? e->s_f64 + e->L.o_color : nullptr;
  r.sref_flags = e->s_i32 ? e->s_i32 + e->L.o_flags : nullptr;
  r.sref_nv = e->s_i32 ? e->s_i32 + e->L.o_nverts : nullptr;
  r.sref_opa = e->s_i32 ? e->s_i32 + e->L.o_opacity : nullptr;
  r.sbg = v.s_bg;
  r.sbg_env_stride = 0; r.env_build = nullptr; r.rgb_override = e->rgb_override;
  r.em = emit_args(e, v); r.draw_ready = 0; r.env0 = 0;
  return r;
}

// Per-env prefix: validates every env's picture against its live record, draws the stale ones again, and points the frame
// launch's arguments at the pictures.  (The launches that do not pass through here --
// anti-aliased canvases -- draw every sprite; the next launch that does re-validates, so nothing goes stale unseen.)
static int use_env_prefix(moog_engine* e, RArgs& r, hipStream_t s) {
  if (e->pe_ns <= 0) return MOOG_OK;
  const int seen = __atomic_load_n(e->pe_min, __ATOMIC_RELAXED);
  if (seen < e->pe_ns) {   // slots from `seen` on do change within episodes: they leave the prefix, every picture is drawn again
    e->pe_ns = seen < 8 ? 0 : seen;
    e->pe_nsv = e->pe_ns > 0 ? e->prog.slot_voff[e->pe_ns] : 0;
    __atomic_store_n(e->pe_min, INT32_MAX, __ATOMIC_RELAXED);
    if (e->pe_ns <= 0) return MOOG_OK;
    HIPCHK(hipMemsetAsync(e->pe_valid, 0, sizeof(int32_t) * (size_t)e->n_envs, s));
  }
  PCArgs c;
  c.P = e->d_prog; c.L = e->L; c.f64 = e->view.f64; c.i32 = e->view.i32; c.s_f64 = e->pe_f64; c.s_i32 = e->pe_i32;
  c.valid = e->pe_valid; c.build = e->pe_build; c.min_changed = e->pe_min; c.n_envs = e->n_envs; c.n_static = e->pe_ns;
  moog_prefix_check_launch(c, s);
  RArgs b = r;
  b.image = e->pe_bg; b.n_static = e->pe_ns; b.nsv = e->pe_nsv; b.build = 1; b.env_build = e->pe_build; b.debug_stop = 0;
  b.sbg = nullptr; b.sbg_env_stride = 0;
  moog_raster_launch(b, e->views[0].raster_lds, s);
  r.n_static = e->pe_ns; r.nsv = e->pe_nsv; r.sbg = e->pe_bg;
  r.sbg_env_stride = (size_t)e->views[0].canvas_h * e->views[0].pad_w * 3;
  return MOOG_OK;
}

// One view's frames: its raster launch (mask or span kernel; the mask kernel derives the draw records first unless draw_ready),
// plus the crop of a 16-aligned canvas or the LANCZOS resize of an anti-aliased one.  Not bracketed: launch_frames times.
static int launch_raster(moog_engine* e, RView& v, uint8_t* image, hipStream_t s, bool draw_ready = false) {
  RArgs r = raster_args(e, v, image);
  r.draw_ready = draw_ready ? 1 : 0;
  if (v.aa <= 1 && &v == &e->views[0]) { const int rc = use_env_prefix(e, r, s); if (rc) return rc; }
  if (v.aa <= 1 && v.pad_w != v.canvas_w) {   // drawn 16-aligned, cropped into the caller's frames
    r.image = v.pad_img;
    moog_raster_launch(r, v.raster_lds, s);
    moog_crop_launch(v.pad_img, image, (size_t)e->n_envs * v.canvas_h, v.pad_w * 3, v.canvas_w * 3, s);
  } else if (v.aa <= 1) {
    moog_raster_launch(r, v.raster_lds, s);
  } else {   // pil_renderer.py:111-112: draw on the large canvas, then Image.resize(LANCZOS); a chunk of envs at a time
    const size_t frame = (size_t)v.render.width * v.render.height * 3;
    for (int e0 = 0; e0 < e->n_envs; e0 += v.aa_chunk) {
      const int n = e->n_envs - e0 < v.aa_chunk ? e->n_envs - e0 : v.aa_chunk;
      RArgs c = r;
      c.f64 = r.f64 + (size_t)e0 * e->L.f64_per_env;
      c.i32 = r.i32 + (size_t)e0 * e->L.i32_per_env;
      c.image = e->aa_canvas;
      c.n_envs = n;
      c.env0 = e0; c.draw_ready = (e0 == 0 && n == e->n_envs) ? r.draw_ready : 0;   // (records derived ahead cover one chunk of every env)
      moog_raster_launch(c, v.raster_lds, s);
      moog_resize_launch(v.aa_resize, e->aa_canvas, e->aa_tmp, image + (size_t)e0 * frame, n, s);
    }
  }
  HIPCHK(hipGetLastError());
  return MOOG_OK;
}

// Whether the draw records of view v can be derived ahead of its raster launch, in the one derive launch of the extra views:
// mask-path frames drawn in one launch over every env (not on top of the per-env prefix: those are the span kernel's).
static bool derives_ahead(moog_engine* e, const RView& v) {
  if (!v.mask_setup.ok || !v.draw) return false;
  if (&v == &e->views[0] && e->pe_ns > 0) return false;
  return v.aa <= 1 || v.aa_chunk >= e->n_envs;
}

// Every bound segmentation of the engine from the records as they are on stream s, under one MOOG_K_VIEWS bracket: one derive
// launch for the draw records of all of them (the emitter with the ids as its per-slot colours, no static prefix), then per
// segmentation the ids kernel and, for a width that is no multiple of 16, the crop.  An engine without a bound segmentation
// returns at the first comparison.
static int launch_segmentations(moog_engine* e, hipStream_t s) {
  if (e->n_bound_segs == 0) return MOOG_OK;
  Bracket br(e, MOOG_K_VIEWS, s);
  RmEmit em[MOOG_MAX_SEGMENTATIONS];
  RArgs r[MOOG_MAX_SEGMENTATIONS];
  SegView* sv[MOOG_MAX_SEGMENTATIONS];
  int n = 0;
  for (int k = 0; k < e->n_segs; ++k) {
    SegView& g = e->segs[k];
    if (!g.ids) continue;
    r[n] = raster_args(e, g.v, g.pad_ids ? g.pad_ids : g.ids);
    r[n].em.rgb_override = g.d_ids; r[n].em.n_static = 0;
    r[n].rgb_override = g.d_ids; r[n].draw_ready = 1;
    em[n] = r[n].em;
    sv[n++] = &g;
  }
  moog_derive_launch(em, n, r[0], s);
  for (int k = 0; k < n; ++k) {
    moog_segmentation_launch(r[k], s);
    const RView& v = sv[k]->v;
    if (sv[k]->pad_ids) moog_crop_launch(sv[k]->pad_ids, sv[k]->ids, (size_t)e->n_envs * v.canvas_h, v.pad_w, v.canvas_w, s);
  }
  HIPCHK(hipGetLastError());
  return MOOG_OK;
}

// Every view's frames of one call: the primary's into `image` (timed as MOOG_K_RASTER, exactly as an engine without extra
// views draws them), then -- under MOOG_K_VIEWS -- one derive launch for the draw records of every extra view on the mask path
// (and of the primary, when its records were not written by the step kernel), the extra views' raster launches, and the
// primary's raster launch behind them.
static int launch_frames(moog_engine* e, uint8_t* image, hipStream_t s, bool draw_ready = false, int timed = -1) {
  { const int rc = launch_segmentations(e, s); if (rc) return rc; }
  RView* extra[MOOG_MAX_VIEWS];
  int n_extra = 0;
  for (int k = 1; k < e->n_views; ++k) if (e->views[k].image) extra[n_extra++] = &e->views[k];
  if (n_extra == 0) {
    Bracket br(e, MOOG_K_RASTER, s, timed);
    return launch_raster(e, e->views[0], image, s, draw_ready);
  }
  RView& p = e->views[0];
  const bool join = !draw_ready && derives_ahead(e, p);   // the primary's records join the extra views' derive launch
  {
    Bracket br(e, MOOG_K_VIEWS, s);
    RmEmit em[MOOG_MAX_VIEWS];
    bool ahead[MOOG_MAX_VIEWS] = {};
    int n_em = 0;
    if (join) em[n_em++] = emit_args(e, p);
    for (int k = 0; k < n_extra; ++k)
      if (derives_ahead(e, *extra[k])) { ahead[k] = true; em[n_em++] = emit_args(e, *extra[k]); }
    if (n_em > 0) moog_derive_launch(em, n_em, raster_args(e, p, image), s);
    for (int k = 0; k < n_extra; ++k) {
      const int rc = launch_raster(e, *extra[k], extra[k]->image, s, ahead[k]);
      if (rc) return rc;
    }
  }
  Bracket br(e, MOOG_K_RASTER, s, timed);
  return launch_raster(e, p, image, s, draw_ready || join);
}

// Every bound sprite table, ray sensor and contacts observer of the engine from the records as they are on stream s: one
// launch for the tables (moog_sprite_table.h), one for the sensors (moog_ray_sensor.h), one for the contacts
// (moog_contacts.h), inside one MOOG_K_TABLES bracket.  An engine without any returns at the first comparison.
enum { OBSERVE_TABLES = 1, OBSERVE_SENSORS = 2, OBSERVE_CONTACTS = 4 };
static int launch_tables(moog_engine* e, hipStream_t s, int what = OBSERVE_TABLES | OBSERVE_SENSORS | OBSERVE_CONTACTS) {
  if (e->tables.n_bound + e->sensors.n_bound + e->contacts.n_bound == 0) return MOOG_OK;
  const bool tables = (what & OBSERVE_TABLES) && e->tables.n_bound, sensors = (what & OBSERVE_SENSORS) && e->sensors.n_bound;
  const bool contacts = (what & OBSERVE_CONTACTS) && e->contacts.n_bound;
  if (!tables && !sensors && !contacts) return MOOG_OK;
  {
    Bracket br(e, MOOG_K_TABLES, s);
    if (tables) {
      StArgs a;
      a.f64 = e->view.f64; a.i32 = e->view.i32;
      a.f64_per_env = e->L.f64_per_env; a.i32_per_env = e->L.i32_per_env;
      a.n_envs = e->n_envs; a.chunk_envs = 0; a.o_flags = e->L.o_flags;
      a.n_tables = gather_bound(e->tables, a.t);
      for (int k = a.n_tables; k < MOOG_MAX_TABLES; ++k) memset(&a.t[k], 0, sizeof a.t[k]);
      moog_sprite_table_launch(a, s);
    }
    if (sensors) {
      RsArgs a;
      moog_rs_args(&e->L, e->view.f64, e->view.i32, e->n_envs, &a);
      a.n_sensors = gather_bound(e->sensors, a.s);
      moog_ray_sensor_launch(a, s);
    }
    if (contacts) {
      CtArgs a;
      moog_ct_args(&e->L, e->view.f64, e->view.i32, e->n_envs, &a);
      a.n_obs = gather_bound(e->contacts, a.c);
      moog_contacts_launch(a, s);
    }
  }
  HIPCHK(hipGetLastError());
  return MOOG_OK;
}

// Reset pool: one fill launch behind the call that has just been enqueued on `s`, on the side streams in turn.  A fill
// serves every env whose pool is empty when it STARTS (not just this call's), so of the launches that pile up on a
// stream behind a fill that is under way (~10 ms of look-ahead per env; calls come every fraction of a millisecond) the
// first does the work and the rest are grids of early exits: each stream always has the next fill ready to start, whether
// the caller synchronises every call or runs hundreds of calls ahead of the device.
// The fill reads the live records while later calls step them: see pool_adopt for why that is sound.
static int pool_kick(moog_engine* e, hipStream_t s) {
  hipStream_t ps = e->pool_stream[e->pool_fills % e->pool_streams];
  HIPCHK(hipEventRecord(e->ev_pool, s));
  HIPCHK(hipStreamWaitEvent(ps, e->ev_pool, 0));
  KArgs a = make_args(e, nullptr, nullptr, nullptr, MODE_FILL, nullptr);
  a.live_f64 = e->view.f64; a.live_i32 = e->view.i32;
  a.f64 = e->pool_f64[1]; a.i32 = e->pool_i32[1];
  a.pool_state = e->pool_state;
  a.fault_flag = nullptr;   // (a fault of the pool's record reaches the host when the record is adopted and stored)
  a.dbg = 0;
  moog_launch_reset_full(e->n_envs * e->pool_depth, e->step_lds, ps, a);   // one workgroup per (record, env)
  HIPCHK(hipGetLastError());
  ++e->pool_fills;
  return MOOG_OK;
}

// Late reset (step_env): behind the step kernel of a program stepped by the kernels without the rare components, the full
// reset kernel opens the episodes of the envs that kernel marked (a grid of early exits when there are none).
static int late_reset_launch(moog_engine* e, const moog_inject_t* inject, const moog_step_out_t* out, hipStream_t s, const RmEmit* draw) {
  KArgs b = make_args(e, nullptr, inject, out, MODE_RESET_MASK, nullptr);
  if (draw) b.draw = *draw;   // (the step launch wrote draw records: the envs this launch resets get theirs from it)
  b.late_mask = e->late_mask;
  b.pool_state = (e->pool_on && !(inject && inject->uniforms)) ? e->pool_state : nullptr;   // (the step kernel took the env's lock then)
  moog_launch_reset_full(e->n_envs, e->step_lds, s, b);
  HIPCHK(hipGetLastError());
  return MOOG_OK;
}

// every pool record is dropped (the host reset the envs, or handed other records over): fills under way finish first
static int pool_drop(moog_engine* e, hipStream_t s) {
  for (int k = 0; k < e->pool_streams; ++k) HIPCHK(hipStreamSynchronize(e->pool_stream[k]));
  HIPCHK(hipMemsetAsync(e->pool_state, 0, sizeof(int32_t) * (size_t)e->n_envs * e->pool_depth, s));
  HIPCHK(hipMemsetAsync(e->pool_lock, 0, sizeof(int32_t) * (size_t)e->n_envs, s));
  return MOOG_OK;
}

static int ready(moog_engine* e) {
  if (!e) return fail(MOOG_E_INVALID, "null engine");
  if (!e->view.f64) return fail(MOOG_E_INVALID, "moog_engine_load_state has not been called");
  HIPCHK(hipSetDevice(e->device));
  return MOOG_OK;
}

int moog_engine_reset(moog_engine_t* e, const uint8_t* env_mask_dev, const moog_inject_t* inject,
                      const moog_step_out_t* out, void* hip_stream) {
  int rc = ready(e);
  if (rc) return rc;
  if (out && out->image && e->frameless) return fail(MOOG_E_INVALID, FRAMELESS_MSG);
  hipStream_t s = (hipStream_t)hip_stream;
  KArgs a = make_args(e, nullptr, inject, out, MODE_RESET_MASK, env_mask_dev);
  if (e->pool_on && (rc = pool_drop(e, s)) != MOOG_OK) return rc;
  {
    Bracket br(e, MOOG_K_RESET, s);
    (e->maze_kernel ? moog_launch_reset_full : moog_launch_reset_plain)(e->n_envs, e->step_lds, s, a);
  }
  HIPCHK(hipGetLastError());
  if (e->pool_on && !(inject && inject->uniforms) && (rc = pool_kick(e, s)) != MOOG_OK) return rc;
  if ((rc = launch_tables(e, s)) != MOOG_OK) return rc;
  if (out && out->image) return launch_frames(e, out->image, s);
  return MOOG_OK;
}

// One MODE_STEP call: moog_engine_step (n_steps = 0: the engine's action repeat, one action block) or
// moog_engine_step_sequence (n_steps >= 1 action blocks act_step_bytes apart, per-step rewards to rewards_dev).
static int step_call(moog_engine* e, const void* actions_dev, int32_t n_steps, int64_t act_step_bytes, double* rewards_dev,
                     int64_t reward_step_elems, const moog_inject_t* inject, const moog_step_out_t* out, void* hip_stream) {
  hipStream_t s = (hipStream_t)hip_stream;
  // (envs whose episode ended in the previous call are reset inside the step kernel, environment.py:100-101)
  KArgs a = make_args(e, actions_dev, inject, out, MODE_STEP, nullptr);
  if (n_steps > 0) {
    a.repeat = n_steps;
    a.act_step_bytes = act_step_bytes;
    a.reward_seq = rewards_dev;
    a.reward_seq_stride = reward_step_elems;
    int n_traj = 0;   // (the tables with a trajectory first: the kernels stop at the first descriptor without a buffer)
    for (int k = 0; k < e->tables.n; ++k)
      if (e->tables.at[k].traj.out) a.traj[n_traj++] = e->tables.at[k].traj;
  }
  int rc;
  const bool emit = out && out->image && step_emits_draw(e);
  if (emit) a.draw = emit_args(e, e->views[0]);
  if (e->sched_pending) {   // the order computed from the previous step's costs
    HIPCHK(hipStreamWaitEvent(s, e->ev_sched_done, 0));
    e->sched_pending = false;
  }
  {
    Bracket br(e, MOOG_K_STEP, s);
    launch_step(e, s, a);
    if (e->late_reset && (rc = late_reset_launch(e, inject, out, s, emit ? &a.draw : nullptr)) != MOOG_OK) return rc;
  }
  HIPCHK(hipGetLastError());
  if (a.pool_state && (rc = pool_kick(e, s)) != MOOG_OK) return rc;
  if (e->perm && e->cost) {
    HIPCHK(hipEventRecord(e->ev_step_done, s));
    HIPCHK(hipStreamWaitEvent(e->sched_stream, e->ev_step_done, 0));
    moog_launch_sched(e->sched_stream, e->cost, e->perm, e->n_envs,
                      e->view.i32 + e->L.o_reset_next, e->L.i32_per_env);
    HIPCHK(hipEventRecord(e->ev_sched_done, e->sched_stream));
    e->sched_pending = true;
  }
  if ((rc = launch_tables(e, s)) != MOOG_OK) return rc;
  if (out && out->image) return launch_frames(e, out->image, s, emit);
  return MOOG_OK;
}

int moog_engine_step(moog_engine_t* e, const void* actions_dev, const moog_inject_t* inject,
                     const moog_step_out_t* out, void* hip_stream) {
  int rc = ready(e);
  if (rc) return rc;
  if (!actions_dev) return fail(MOOG_E_INVALID, "null actions");
  if (out && out->image && e->frameless) return fail(MOOG_E_INVALID, FRAMELESS_MSG);
  if (e->action_repeat > 1 && inject && inject->uniforms)
    return fail(MOOG_E_UNSUPPORTED, "injected uniforms are one call's stream: they cannot feed the several env-steps of an action repeat (moog_engine_set_action_repeat(e, 1, ...) first)");
  return step_call(e, actions_dev, 0, 0, nullptr, 0, inject, out, hip_stream);
}

int moog_engine_step_sequence(moog_engine_t* e, const void* actions_dev, int32_t n_steps, int64_t action_step_bytes,
                              double* rewards_dev, int64_t reward_step_elems, const moog_inject_t* inject,
                              const moog_step_out_t* out, void* hip_stream) {
  int rc = ready(e);
  if (rc) return rc;
  if (!actions_dev) return fail(MOOG_E_INVALID, "null actions");
  if (!rewards_dev) return fail(MOOG_E_INVALID, "null rewards");
  if (n_steps < 1 || n_steps > MOOG_MAX_ACTION_REPEAT)
    return fail(MOOG_E_INVALID, "sequence length out of range (1 .. MOOG_MAX_ACTION_REPEAT)");
  if (out && out->image && e->frameless) return fail(MOOG_E_INVALID, FRAMELESS_MSG);
  if (inject && inject->uniforms)
    return fail(MOOG_E_UNSUPPORTED, "injected uniforms are one env-step's stream: they cannot feed the env-steps of an action sequence (moog_engine_step takes them)");
  if (e->action_repeat > 1)
    return fail(MOOG_E_UNSUPPORTED, "an action sequence on an engine with an action repeat above 1 (a hold count per entry) is not available: moog_engine_set_action_repeat(e, 1, ...) first");
  return step_call(e, actions_dev, n_steps, action_step_bytes, rewards_dev, reward_step_elems, inject, out, hip_stream);
}

static bool plans_specialised(const moog_engine* e) { return e->spec_plan_launch && e->step_dbg == 0 && !e->watch; }

int moog_engine_plan_sequences(moog_engine_t* e, const void* actions_dev, int32_t n_cand, int32_t n_steps,
                               int64_t action_cand_bytes, int64_t action_step_bytes, double* rewards_dev,
                               int64_t reward_cand_elems, int64_t reward_step_elems, int32_t* count_dev, uint8_t* ended_dev,
                               int64_t count_cand_elems, const int64_t* traj_cand_elems, void* hip_stream) {
  int rc = ready(e);
  if (rc) return rc;
  if (!actions_dev) return fail(MOOG_E_INVALID, "null actions");
  if (!rewards_dev) return fail(MOOG_E_INVALID, "null rewards");
  if (!count_dev || !ended_dev) return fail(MOOG_E_INVALID, "null count / ended");
  if (n_cand < 1 || n_cand > MOOG_MAX_PLAN_CANDIDATES)
    return fail(MOOG_E_INVALID, "candidate count out of range (1 .. MOOG_MAX_PLAN_CANDIDATES)");
  if (n_steps < 1 || n_steps > MOOG_MAX_ACTION_REPEAT)
    return fail(MOOG_E_INVALID, "sequence length out of range (1 .. MOOG_MAX_ACTION_REPEAT)");
  if (action_cand_bytes < 0 || action_step_bytes < 0 || reward_step_elems < e->n_envs ||
      reward_cand_elems < (int64_t)(n_steps - 1) * reward_step_elems + e->n_envs || count_cand_elems < e->n_envs)
    return fail(MOOG_E_INVALID, "candidate rollouts: a stride is shorter than the block it steps over");
  if ((int64_t)e->n_envs * n_cand > 0x7fffffffll) return fail(MOOG_E_INVALID, "candidate rollouts: n_envs x n_cand exceeds the grid");
  if (e->action_repeat > 1)
    return fail(MOOG_E_UNSUPPORTED, "candidate rollouts on an engine with an action repeat above 1 (a hold count per entry) are not available: moog_engine_set_action_repeat(e, 1, ...) first");
  if (!e->plan_lds) return fail(MOOG_E_UNSUPPORTED, "candidate rollouts stage the whole record: this program's does not fit in 160 KB of LDS with the fields the step kernels leave in HBM");
  hipStream_t s = (hipStream_t)hip_stream;
  // MODE_STEP arguments, then everything a candidate must not touch taken out: no outputs, no cost, no pool, no late mask, no
  // count buffer, no watcher, no usage counters, no draw record; the record's layout in LDS is the uncut one
  KArgs a = make_args(e, actions_dev, nullptr, nullptr, MODE_STEP, nullptr);
  a.H = hot_layout_uncut(e->L);
  a.xstack_off = e->plan_xstack_off;
  a.cost = nullptr; a.pool_state = nullptr; a.late_mask = nullptr; a.repeat_count = nullptr; a.watch = nullptr;
  a.layer_hw = nullptr; a.fault_flag = nullptr;
  a.repeat = n_steps;
  a.act_step_bytes = action_step_bytes;
  a.reward_seq = rewards_dev;
  a.reward_seq_stride = reward_step_elems;
  a.n_cand = n_cand;
  a.act_cand_bytes = action_cand_bytes;
  a.reward_cand_stride = reward_cand_elems;
  a.plan_count = count_dev; a.plan_ended = ended_dev; a.count_cand_stride = count_cand_elems;
  int n_traj = 0;   // (the tables with a trajectory first, as in step_call)
  for (int k = 0; k < e->tables.n; ++k) {
    const TrajTable& t = e->tables.at[k].traj;
    if (!t.out) continue;
    const int64_t block = (int64_t)e->n_envs * t.n_rows * (int64_t)t.n_cols;
    if (!traj_cand_elems || traj_cand_elems[k] < (int64_t)(n_steps - 1) * t.step_elems + block)
      return fail(MOOG_E_INVALID, "candidate rollouts: a bound trajectory needs its candidate stride (traj_cand_elems[table] >= (n_steps - 1) x step_elems + n_envs x n_rows x n_cols)");
    a.traj_cand_elems[n_traj] = traj_cand_elems[k];
    a.traj[n_traj++] = t;
  }
  if (e->sched_pending) HIPCHK(hipStreamWaitEvent(s, e->ev_sched_done, 0));   // (the launch order is read: not while the sort writes it)
  {
    Bracket br(e, MOOG_K_STEP, s);
    const int blocks = e->n_envs * n_cand;
    if (plans_specialised(e)) e->spec_plan_launch(blocks, e->plan_lds, s, &a);
    else {
      static const moog_step_launch_fn launch[6] = {moog_launch_step_f3rp, moog_launch_step_f4rp, moog_launch_step_t3rp,
                                                    moog_launch_step_t4rp, moog_launch_step_m3rp, moog_launch_step_m4rp};
      const bool full = e->maze_kernel && !e->late_reset;
      launch[(full ? 4 : (e->dynamic_rules ? 2 : 0)) + (e->step_wps == 4 ? 1 : 0)](blocks, e->plan_lds, s, a);
    }
  }
  HIPCHK(hipGetLastError());
  return MOOG_OK;
}

int moog_engine_plan_kernel(moog_engine_t* e, int32_t* specialised) {
  if (!e || !specialised) return fail(MOOG_E_INVALID, "null argument");
  *specialised = plans_specialised(e) ? 1 : 0;
  return MOOG_OK;
}

int moog_engine_physics_only(moog_engine_t* e, const moog_inject_t* inject, void* hip_stream) {
  int rc = ready(e);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  KArgs a = make_args(e, nullptr, inject, nullptr, MODE_PHYSICS, nullptr);
  {
    Bracket br(e, MOOG_K_STEP, s);
    launch_step(e, s, a);
  }
  HIPCHK(hipGetLastError());
  return MOOG_OK;
}

int moog_engine_render(moog_engine_t* e, uint8_t* image_dev, void* hip_stream) {
  int rc = ready(e);
  if (rc) return rc;
  if (!image_dev) return fail(MOOG_E_INVALID, "null image");
  if (e->frameless) return fail(MOOG_E_INVALID, FRAMELESS_MSG);
  return launch_frames(e, image_dev, (hipStream_t)hip_stream);
}

int moog_engine_set_schedule(moog_engine_t* e, int32_t* perm_dev, float* cost_dev) {
  if (!e) return fail(MOOG_E_INVALID, "null engine");
  if (e->sched_pending) { hipEventSynchronize(e->ev_sched_done); e->sched_pending = false; }
  e->perm = perm_dev;
  e->cost = cost_dev;
  if (perm_dev && cost_dev) {   // the step kernel reads the costs (a moving average): they start from zero, whatever the caller's memory held
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemset(cost_dev, 0, (size_t)e->n_envs * sizeof(float)));
  }
  if (perm_dev && cost_dev && !e->sched_stream) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamCreateWithFlags(&e->sched_stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&e->ev_step_done, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&e->ev_sched_done, hipEventDisableTiming));
  }
  return MOOG_OK;
}

int moog_engine_set_reset_pool(moog_engine_t* e, int32_t enabled) {
  if (!e) return fail(MOOG_E_INVALID, "null engine");
  HIPCHK(hipSetDevice(e->device));
  if (!enabled) {
    if (e->pool_on) { const int rc = pool_drop(e, 0); if (rc) return rc; HIPCHK(hipStreamSynchronize(0)); }
    e->pool_on = false;
    return MOOG_OK;
  }
  if (!e->maze_kernel)
    return fail(MOOG_E_UNSUPPORTED, "the reset pool lives in the kernels that carry every component; this program runs the plain ones (its resets are cheap)");
  for (int o = 0; o < e->prog.n_ops; ++o)
    if (e->prog.ops[o].cell_sel == MOOG_CELL_PSTATE)
      return fail(MOOG_E_UNSUPPORTED, "the reset pool cannot serve a program whose initializer keeps a number across episodes (MOOG_CELL_PSTATE): its resets depend on how the previous episode went");
  {
    const char* ser = getenv("AMD_SERIALIZE_KERNEL");
    const char* blk = getenv("HIP_LAUNCH_BLOCKING");
    const char* hwq = getenv("GPU_MAX_HW_QUEUES");
    const char* cc = getenv("ROCPROF_COUNTER_COLLECTION");
    if ((ser && atoi(ser)) || (blk && atoi(blk)) || (hwq && atoi(hwq) == 1) || (cc && atoi(cc)))
      return fail(MOOG_E_UNSUPPORTED, "the reset pool needs kernels to run beside each other (AMD_SERIALIZE_KERNEL / HIP_LAUNCH_BLOCKING / GPU_MAX_HW_QUEUES=1 / counter collection serialise them)");
  }
  if (!e->pool_ready) {
    const size_t n = (size_t)e->n_envs * e->pool_depth;
    if (!e->pool_state) HIPCHK(hipMalloc(&e->pool_state, sizeof(int32_t) * n));
    if (!e->pool_tag) HIPCHK(hipMalloc(&e->pool_tag, sizeof(int32_t) * n));
    if (!e->pool_lock) HIPCHK(hipMalloc(&e->pool_lock, sizeof(int32_t) * (size_t)e->n_envs));
    if (!e->pool_stats) { HIPCHK(hipMalloc(&e->pool_stats, 4 * sizeof(unsigned long long))); HIPCHK(hipMemset(e->pool_stats, 0, 4 * sizeof(unsigned long long))); }
    for (int k = 0; k < 2; ++k) {
      if (!e->pool_f64[k]) HIPCHK(hipMalloc(&e->pool_f64[k], sizeof(double) * n * (size_t)e->L.f64_per_env));
      if (!e->pool_i32[k]) HIPCHK(hipMalloc(&e->pool_i32[k], sizeof(int32_t) * n * (size_t)e->L.i32_per_env));
    }
    {   // streams that share a hardware queue with the caller's would put its step kernels behind a fill
      const char* hwq = getenv("GPU_MAX_HW_QUEUES");
      const int queues = (hwq && atoi(hwq) > 0) ? atoi(hwq) : 4;
      e->pool_streams = queues - 2 < 1 ? 1 : (queues - 2 > moog_engine::POOL_STREAMS ? moog_engine::POOL_STREAMS : queues - 2);
    }
    for (int k = 0; k < e->pool_streams; ++k)
      if (!e->pool_stream[k]) HIPCHK(hipStreamCreateWithFlags(&e->pool_stream[k], hipStreamNonBlocking));
    if (!e->ev_pool) HIPCHK(hipEventCreateWithFlags(&e->ev_pool, hipEventDisableTiming));
    e->pool_ready = true;
  }
  HIPCHK(hipMemset(e->pool_state, 0, sizeof(int32_t) * (size_t)e->n_envs * e->pool_depth));
  HIPCHK(hipMemset(e->pool_tag, 0, sizeof(int32_t) * (size_t)e->n_envs * e->pool_depth));
  HIPCHK(hipMemset(e->pool_lock, 0, sizeof(int32_t) * (size_t)e->n_envs));
  e->pool_on = true;
  return MOOG_OK;
}

int moog_engine_get_reset_pool(moog_engine_t* e, int32_t* enabled, int64_t* stats) {
  if (!e) return fail(MOOG_E_INVALID, "null engine");
  if (enabled) *enabled = e->pool_on ? 1 : 0;
  if (stats) {
    stats[0] = e->pool_fills;
    for (int k = 1; k < 5; ++k) stats[k] = 0;
    if (e->pool_stats) {   // (synchronises the device)
      unsigned long long h[4];
      HIPCHK(hipSetDevice(e->device));
      HIPCHK(hipDeviceSynchronize());
      HIPCHK(hipMemcpy(h, e->pool_stats, sizeof(h), hipMemcpyDeviceToHost));
      for (int k = 0; k < 4; ++k) stats[1 + k] = (int64_t)h[k];
    }
  }
  return MOOG_OK;
}

int moog_engine_set_action_dtype(moog_engine_t* e, int32_t float32) {
  if (!e) return fail(MOOG_E_INVALID, "null engine");
  e->act_f32 = float32 ? 1 : 0;
  return MOOG_OK;
}

int moog_engine_set_action_repeat(moog_engine_t* e, int32_t k, int32_t* count_dev) {
  if (!e) return fail(MOOG_E_INVALID, "null engine");
  if (k < 1 || k > MOOG_MAX_ACTION_REPEAT) return fail(MOOG_E_INVALID, "action repeat out of range (1 .. MOOG_MAX_ACTION_REPEAT)");
  e->action_repeat = k;
  e->repeat_count = count_dev;
  return MOOG_OK;
}

int moog_engine_layer_usage(moog_engine_t* e, int32_t* high_water, int32_t* dropped) {
  if (!e || !high_water || !dropped) return fail(MOOG_E_INVALID, "null argument");
  int32_t host[2 * MOOG_MAX_LAYERS] = {0};
  if (e->layer_hw) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpy(host, e->layer_hw, sizeof(host), hipMemcpyDeviceToHost));   // (synchronises with the null stream's work)
  }
  for (int l = 0; l < MOOG_MAX_LAYERS; ++l) { high_water[l] = host[l]; dropped[l] = host[MOOG_MAX_LAYERS + l]; }
  return MOOG_OK;
}

int moog_program_step_kernel(const moog_program_t* prog, int32_t* variant, int32_t* wps, uint64_t* hash) {
  if (!prog) return fail(MOOG_E_INVALID, "null program");
  const StepVariant v = step_variant_of(prog);
  if (variant) *variant = (v.maze_kernel && !v.late_reset) ? 2 : (v.dynamic_rules ? 1 : 0);
  if (wps) *wps = v.wps;
  if (hash) *hash = program_hash(prog);
  return MOOG_OK;
}

int moog_engine_step_kernel(moog_engine_t* e, int32_t* specialised) {
  if (!e || !specialised) return fail(MOOG_E_INVALID, "null argument");
  *specialised = steps_specialised(e) ? 1 : 0;
  return MOOG_OK;
}

int moog_engine_read_draw_records(moog_engine_t* e, uint8_t* host_out, int64_t bytes, int64_t* stride, int32_t* in_step) {
  if (!e) return fail(MOOG_E_INVALID, "null engine");
  const RView& v = e->views[0];
  if (!v.mask_setup.ok || !v.draw) return fail(MOOG_E_UNSUPPORTED, "this program's frames are not the mask rasteriser's: no draw records");
  if (stride) *stride = (int64_t)v.draw_lay.stride;
  if (in_step) *in_step = step_emits_draw(e) ? 1 : 0;
  if (!host_out) return MOOG_OK;
  const int64_t need = (int64_t)e->n_envs * (int64_t)v.draw_lay.stride;
  if (bytes < need) return fail(MOOG_E_INVALID, "host buffer too small for the draw records");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host_out, v.draw, (size_t)need, hipMemcpyDeviceToHost));
  return MOOG_OK;
}

int moog_engine_raster_path(moog_engine_t* e, int32_t* path) { return moog_engine_view_raster_path(e, 0, path); }

int moog_engine_view_raster_path(moog_engine_t* e, int32_t view, int32_t* path) {
  if (!e || !path) return fail(MOOG_E_INVALID, "null argument");
  if (e->frameless) return fail(MOOG_E_INVALID, FRAMELESS_MSG);
  if (view < 0 || view >= e->n_views) return fail(MOOG_E_INVALID, "no such view");
  const RmSetup& ms = e->views[view].mask_setup;
  const bool prefix = view == 0 && e->pe_ns > 0;   // (frames on top of the per-env prefix are the span kernel's)
  *path = (ms.ok && !prefix) ? (ms.compact ? MOOG_RASTER_MASK_COMPACT : MOOG_RASTER_MASK) : MOOG_RASTER_SPANS;
  return MOOG_OK;
}

int moog_engine_add_view(moog_engine_t* e, const moog_render_t* render, int32_t* view) {
  if (!e || !render || !view) return fail(MOOG_E_INVALID, "null argument");
  if (e->frameless) return fail(MOOG_E_INVALID, "this program draws no frames (render 0 x 0): it takes no extra views");
  if (e->n_views >= MOOG_MAX_VIEWS) return fail(MOOG_E_UNSUPPORTED, "at most MOOG_MAX_VIEWS views per engine");
  int rc = validate_render(&e->prog, render);
  if (rc) return rc;
  HIPCHK(hipSetDevice(e->device));
  RView& v = e->views[e->n_views];
  v = RView();
  v.render = *render;
  moog_program_t* host = new moog_program_t(e->prog);   // (the span kernel reads P->render: a device program of the view's own)
  host->render = *render;
  hipError_t err = hipMalloc(&v.d_own, sizeof(moog_program_t));
  if (err == hipSuccess) err = hipMemcpy(v.d_own, host, sizeof(moog_program_t), hipMemcpyHostToDevice);
  delete host;
  v.P = v.d_own;
  if (err == hipSuccess) rc = setup_view(e, v, false);
  else rc = fail(MOOG_E_NOMEM, "hipMalloc(view program) failed");
  if (rc == MOOG_OK) rc = build_static_prefix(e, v);
  if (rc == MOOG_OK) rc = setup_anti_aliasing(e, v);
  if (rc == MOOG_OK && v.aa <= 1 && v.pad_w != v.canvas_w &&
      hipMalloc(&v.pad_img, (size_t)e->n_envs * v.canvas_h * v.pad_w * 3) != hipSuccess)
    rc = fail(MOOG_E_NOMEM, "hipMalloc(16-aligned frames) failed");
  if (rc == MOOG_OK) {   // (the kernels' LDS limit is process-wide and only grows: moog_raster_configure)
    err = (hipError_t)moog_raster_configure(v.raster_lds);
    if (err == hipSuccess && v.mask_setup.ok) err = (hipError_t)moog_raster_configure_mask(64 * 1024);
    if (err != hipSuccess) rc = fail(MOOG_E_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(err));
  }
  if (rc == MOOG_OK && e->rgb_override) { v.kept_n_static = v.n_static; v.n_static = 0; }
  if (rc) {
    const std::string msg = g_err;
    if (v.d_own) hipFree(v.d_own);
    if (v.draw) hipFree(v.draw);
    if (v.s_bg) hipFree(v.s_bg);
    if (v.pad_img) hipFree(v.pad_img);
    if (v.aa_tables) hipFree(v.aa_tables);
    if (v.rows_seen) hipHostFree(v.rows_seen);
    v = RView();
    g_err = msg;
    return rc;
  }
  *view = e->n_views++;
  return MOOG_OK;
}

int moog_engine_set_view_image(moog_engine_t* e, int32_t view, uint8_t* image_dev) {
  if (!e) return fail(MOOG_E_INVALID, "null engine");
  if (view < 1 || view >= e->n_views) return fail(MOOG_E_INVALID, "no such extra view (the primary's frames are the calls' own image)");
  e->views[view].image = image_dev;
  return MOOG_OK;
}

int moog_engine_add_segmentation(moog_engine_t* e, const moog_segmentation_t* seg, int32_t* index) {
  if (!e || !seg || !index) return fail(MOOG_E_INVALID, "null argument");
  if (e->frameless) return fail(MOOG_E_INVALID, "this program draws no frames (render 0 x 0): its engine has no raster state and takes no segmentation");
  if (e->n_segs >= MOOG_MAX_SEGMENTATIONS) return fail(MOOG_E_UNSUPPORTED, "at most MOOG_MAX_SEGMENTATIONS segmentations per engine");
  if (seg->width < 1 || seg->width > 128 || seg->height < 1 || seg->height > 128)
    return fail(MOOG_E_INVALID, "segmentation size out of range (1 <= height, width <= 128: larger frames are the span rasteriser's, which draws no ids)");
  if (seg->n_slots != e->prog.n_slots) return fail(MOOG_E_INVALID, "segmentation n_slots is not the program's");
  moog_render_t render;
  memset(&render, 0, sizeof render);
  render.width = seg->width; render.height = seg->height; render.cmap = MOOG_CMAP_IDENTITY; render.aa = 1;
  render.polymod = seg->polymod; render.polymod_layer = seg->polymod_layer;
  int rc = validate_render(&e->prog, &render);
  if (rc) return rc;
  HIPCHK(hipSetDevice(e->device));
  SegView& g = e->segs[e->n_segs];
  g = SegView();
  g.v.render = render;
  g.v.P = e->d_prog;   // (the emitter reads the slots' vertex offsets from it; `render` is the span kernel's business)
  rc = setup_view(e, g.v, false);
  if (rc == MOOG_OK && !g.v.mask_setup.ok)
    rc = fail(MOOG_E_UNSUPPORTED, "a frame of this size and modifier is not the mask rasteriser's (more than 256 items, or tables beyond 64 KB of LDS): no segmentation");
  if (rc == MOOG_OK) {
    const size_t slots = (size_t)e->prog.n_slots;
    std::vector<uint32_t> ids((size_t)e->n_envs * slots);
    for (size_t env = 0; env < (size_t)e->n_envs; ++env)
      for (size_t sl = 0; sl < slots; ++sl) ids[env * slots + sl] = seg->slot_id[sl];
    if (hipMalloc(&g.d_ids, ids.size() * sizeof(uint32_t)) != hipSuccess ||
        hipMemcpy(g.d_ids, ids.data(), ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(MOOG_E_NOMEM, "hipMalloc(segmentation ids) failed");
  }
  if (rc == MOOG_OK && g.v.pad_w != g.v.canvas_w &&
      hipMalloc(&g.pad_ids, (size_t)e->n_envs * g.v.canvas_h * g.v.pad_w) != hipSuccess)
    rc = fail(MOOG_E_NOMEM, "hipMalloc(16-aligned segmentation) failed");
  if (rc == MOOG_OK) {   // (the kernels' LDS limit is process-wide and only grows: moog_raster_configure_mask)
    const hipError_t err = (hipError_t)moog_raster_configure_mask(64 * 1024);
    if (err != hipSuccess) rc = fail(MOOG_E_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(err));
  }
  if (rc) {
    const std::string msg = g_err;
    (void)hipGetLastError();
    if (g.v.draw) hipFree(g.v.draw);
    if (g.v.rows_seen) hipHostFree(g.v.rows_seen);
    if (g.d_ids) hipFree(g.d_ids);
    if (g.pad_ids) hipFree(g.pad_ids);
    g = SegView();
    g_err = msg;
    return rc;
  }
  *index = e->n_segs++;
  return MOOG_OK;
}

int moog_engine_set_segmentation_image(moog_engine_t* e, int32_t index, uint8_t* ids_dev) {
  if (!e) return fail(MOOG_E_INVALID, "null engine");
  if (index < 0 || index >= e->n_segs) return fail(MOOG_E_INVALID, "no such segmentation");
  SegView& g = e->segs[index];
  if (!g.pad_ids && ((uintptr_t)ids_dev & 15))   // (the ids kernel stores 16 pixels at a time straight into it)
    return fail(MOOG_E_INVALID, "segmentation image must be 16-byte aligned");
  e->n_bound_segs += (ids_dev ? 1 : 0) - (g.ids ? 1 : 0);
  g.ids = ids_dev;
  return MOOG_OK;
}

// ---- sprite tables, ray sensors, contacts observers: add / set buffer / observe (the helpers are above free_engine) ------------
int moog_engine_add_table(moog_engine_t* e, const moog_table_t* table_desc, int32_t* table) {
  STable* t;
  int rc = next_observer(e, &moog_engine::tables, table_desc, table, "at most MOOG_MAX_TABLES sprite tables per engine", &t);
  if (rc) return rc;
  int32_t rows[MOOG_MAX_SLOTS];
  StTable d;
  memset(&d, 0, sizeof d);
  const char* why = moog_st_describe(&e->prog, &e->L, table_desc, &d, rows);
  if (why) return fail(MOOG_E_INVALID, why);
  const Upload up[] = {{rows, sizeof(int32_t) * (size_t)table_desc->n_rows}};
  rc = upload_observer(e, up, 1, t->d_mem);
  if (rc) return rc;
  d.rows = (const int32_t*)t->d_mem[0];
  t->desc = d;
  memset(&t->traj, 0, sizeof t->traj);
  t->traj.rows = d.rows;
  t->traj.n_rows = table_desc->n_rows;
  t->traj.n_cols = (uint8_t)table_desc->n_cols;
  t->traj.dtype = (uint8_t)table_desc->dtype;
  for (int c = 0; c < table_desc->n_cols; ++c) t->traj.cols[c / 8] |= (uint64_t)(uint8_t)table_desc->cols[c] << (8 * (c % 8));
  *table = e->tables.n++;
  return MOOG_OK;
}

int moog_engine_set_table_buffer(moog_engine_t* e, int32_t table, void* table_dev) {
  return bind_observer(e, &moog_engine::tables, table, table_dev, "no such sprite table",
                       [](const StTable& d) -> uintptr_t { return d.dtype == MOOG_TABLE_F16 ? 1u : 3u; },
                       "sprite table buffer must be aligned to its element type");
}

int moog_engine_set_table_trajectory(moog_engine_t* e, int32_t table, void* traj_dev, int64_t step_elems) {
  if (!e) return fail(MOOG_E_INVALID, "null engine");
  if (table < 0 || table >= e->tables.n) return fail(MOOG_E_INVALID, "no such sprite table");
  TrajTable& t = e->tables.at[table].traj;
  if ((uintptr_t)traj_dev & (t.dtype == MOOG_TABLE_F16 ? 1u : 3u))
    return fail(MOOG_E_INVALID, "sprite table trajectory must be aligned to its element type");
  if (traj_dev && step_elems < (int64_t)e->n_envs * t.n_rows * (int64_t)t.n_cols)
    return fail(MOOG_E_INVALID, "sprite table trajectory: step_elems is less than one step's block (n_envs x n_rows x n_cols)");
  t.out = traj_dev;
  t.step_elems = traj_dev ? step_elems : 0;
  return MOOG_OK;
}

int moog_engine_observe_tables(moog_engine_t* e, void* hip_stream) {
  const int rc = ready(e);
  if (rc) return rc;
  return launch_tables(e, (hipStream_t)hip_stream, OBSERVE_TABLES);
}

int moog_engine_add_sensor(moog_engine_t* e, const moog_sensor_t* sensor_desc, int32_t* sensor) {
  Attached<RsSensor>* t;
  int rc = next_observer(e, &moog_engine::sensors, sensor_desc, sensor, "at most MOOG_MAX_SENSORS ray sensors per engine", &t);
  if (rc) return rc;
  int32_t rows[3 * MOOG_MAX_SLOTS];
  RsSensor d;
  memset(&d, 0, sizeof d);
  const char* why = moog_rs_describe(&e->prog, &e->L, sensor_desc, &d, rows);
  if (why) return fail(MOOG_E_INVALID, why);
  const Upload up[] = {{rows, sizeof(int32_t) * 3 * (size_t)sensor_desc->n_rows},
                       {sensor_desc->dirs, sizeof(double) * 2 * (size_t)sensor_desc->n_rays}};
  rc = upload_observer(e, up, 2, t->d_mem);
  if (rc) return rc;
  d.rows = (const int32_t*)t->d_mem[0];
  d.dirs = (const double*)t->d_mem[1];
  t->desc = d;
  *sensor = e->sensors.n++;
  return MOOG_OK;
}

int moog_engine_set_sensor_buffer(moog_engine_t* e, int32_t sensor, void* sensor_dev) {
  return bind_observer(e, &moog_engine::sensors, sensor, sensor_dev, "no such ray sensor",
                       [](const RsSensor&) -> uintptr_t { return 3u; },
                       "ray sensor buffer must be 4-byte aligned (a float16 ray is one dword)");
}

int moog_engine_observe_sensors(moog_engine_t* e, void* hip_stream) {
  const int rc = ready(e);
  if (rc) return rc;
  return launch_tables(e, (hipStream_t)hip_stream, OBSERVE_SENSORS);
}

int moog_engine_add_contacts(moog_engine_t* e, const moog_contacts_t* contacts_desc, int32_t* contacts) {
  Attached<CtObs>* t;
  int rc = next_observer(e, &moog_engine::contacts, contacts_desc, contacts,
                         "at most MOOG_MAX_CONTACTS contacts observers per engine", &t);
  if (rc) return rc;
  int32_t rows[3 * 2 * MOOG_MAX_SLOTS];
  CtObs d;
  memset(&d, 0, sizeof d);
  const char* why = moog_ct_describe(&e->prog, &e->L, contacts_desc, &d, rows);
  if (why) return fail(MOOG_E_INVALID, why);
  const Upload up[] = {{rows, sizeof(int32_t) * 3 * ((size_t)contacts_desc->n_rows_0 + (size_t)contacts_desc->n_rows_1)}};
  rc = upload_observer(e, up, 1, t->d_mem);
  if (rc) return rc;
  d.rows = (const int32_t*)t->d_mem[0];
  t->desc = d;
  *contacts = e->contacts.n++;
  return MOOG_OK;
}

int moog_engine_set_contacts_buffer(moog_engine_t* e, int32_t contacts, void* contacts_dev) {
  // (no alignment asked: the kernel stores bytes up to the first dword boundary of an env's block)
  return bind_observer(e, &moog_engine::contacts, contacts, contacts_dev, "no such contacts observer",
                       [](const CtObs&) -> uintptr_t { return 0u; }, "");
}

int moog_engine_observe_contacts(moog_engine_t* e, void* hip_stream) {
  const int rc = ready(e);
  if (rc) return rc;
  return launch_tables(e, (hipStream_t)hip_stream, OBSERVE_CONTACTS);
}

int moog_engine_kernel_variant(moog_engine_t* e, int32_t* variant, int32_t* late_reset) {
  if (!e) return fail(MOOG_E_INVALID, "null engine");
  const bool full = e->maze_kernel && !e->late_reset;
  if (variant) *variant = full ? 2 : (e->dynamic_rules ? 1 : 0);
  if (late_reset) *late_reset = e->late_reset ? 1 : 0;
  return MOOG_OK;
}

int moog_engine_set_color_override(moog_engine_t* e, const uint32_t* rgb_dev) {
  if (!e) return fail(MOOG_E_INVALID, "null engine");
  if (rgb_dev && !e->rgb_override) {   // the cached pictures hold the colour map's colours: off while the host supplies them
    for (int k = 0; k < e->n_views; ++k) { e->views[k].kept_n_static = e->views[k].n_static; e->views[k].n_static = 0; }
    e->kept_pe_ns = e->pe_ns; e->kept_pe_nsv = e->pe_nsv;
    e->pe_ns = 0; e->pe_nsv = 0;
  } else if (!rgb_dev && e->rgb_override) {   // back to render.cmap: the prefixes as they were (the per-env pictures are drawn again)
    for (int k = 0; k < e->n_views; ++k) e->views[k].n_static = e->views[k].kept_n_static;
    e->pe_ns = e->kept_pe_ns; e->pe_nsv = e->kept_pe_nsv;
    if (e->pe_ns > 0 && e->pe_valid) HIPCHK(hipMemset(e->pe_valid, 0, sizeof(int32_t) * (size_t)e->n_envs));
  }
  e->rgb_override = rgb_dev;
  return MOOG_OK;
}

int moog_engine_env_prefix(moog_engine_t* e, int32_t* n_slots) {
  if (!e || !n_slots) return fail(MOOG_E_INVALID, "null argument");
  int ns = e->pe_ns;
  if (ns > 0) { const int seen = __atomic_load_n(e->pe_min, __ATOMIC_RELAXED); if (seen < ns) ns = seen < 8 ? 0 : seen; }
  *n_slots = ns;
  return MOOG_OK;
}

int moog_engine_static_prefix(moog_engine_t* e, int32_t* n_slots, uint8_t* image_dev, void* hip_stream) {
  if (!e) return fail(MOOG_E_INVALID, "null engine");
  const RView& v = e->views[0];
  if (n_slots) *n_slots = v.n_static;
  if (image_dev && v.n_static > 0) {
    HIPCHK(hipSetDevice(e->device));
    if (v.aa > 1) return fail(MOOG_E_UNSUPPORTED, "the cached picture of an anti-aliased renderer is canvas sized");
    if (v.pad_w != v.canvas_w)
      moog_crop_launch(v.s_bg, image_dev, (size_t)v.canvas_h, v.pad_w * 3, v.canvas_w * 3, (hipStream_t)hip_stream);
    else
      HIPCHK(hipMemcpyAsync(image_dev, v.s_bg, (size_t)v.render.width * v.render.height * 3,
                            hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
  }
  return MOOG_OK;
}

int moog_engine_poll_faults(moog_engine_t* e, int32_t clear, int32_t* bits) {
  if (!e || !bits) return fail(MOOG_E_INVALID, "null argument");
  *bits = __atomic_load_n(e->fault_flag, __ATOMIC_RELAXED);   // no stream synchronisation: what has arrived so far
  if (clear && *bits) __atomic_and_fetch(e->fault_flag, ~*bits, __ATOMIC_RELAXED);
  return MOOG_OK;
}

int moog_engine_set_debug(moog_engine_t* e, int32_t step_debug, int32_t raster_stop) {
  if (!e) return fail(MOOG_E_INVALID, "null engine");
  e->step_dbg = step_debug;
  e->raster_stop = raster_stop;
  return MOOG_OK;
}

int moog_engine_read_watch(moog_engine_t* e, int32_t* host_out, int32_t clear) {
  if (!e || !host_out) return fail(MOOG_E_INVALID, "null argument");
  if (!e->watch) return fail(MOOG_E_UNSUPPORTED, "section sampling needs an engine created with MOOG_WATCH=1");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  const size_t bytes = (size_t)e->n_envs * MOOG_WATCH_SECTIONS * sizeof(int32_t);
  HIPCHK(hipMemcpy(host_out, e->watch, bytes, hipMemcpyDeviceToHost));
  if (clear) HIPCHK(hipMemset(e->watch, 0, bytes));
  return MOOG_OK;
}

int moog_engine_set_timing(moog_engine_t* e, int32_t enabled) {
  if (!e) return fail(MOOG_E_INVALID, "null engine");
  e->timing = enabled;
  return MOOG_OK;
}

int moog_engine_kernel_time(moog_engine_t* e, int32_t kernel_id, double* total_ms, int64_t* launches) {
  if (!e || kernel_id < 0 || kernel_id >= MOOG_K_COUNT) return fail(MOOG_E_INVALID, "bad kernel id");
  drain(e->timed[kernel_id]);
  if (total_ms) *total_ms = e->timed[kernel_id].total_ms;
  if (launches) *launches = e->timed[kernel_id].launches;
  e->timed[kernel_id].total_ms = 0;
  e->timed[kernel_id].launches = 0;
  return MOOG_OK;
}

}  // extern "C"

// One object of the spec directory: <prefix>_<hash>_d<variant>w<wps>.so, its configure function called with `lds`.  Returns the
// launch function (and the handle), or null with the reason on stderr.
static void* load_spec_object(moog_engine* e, const moog_program_t* prog, const char* prefix, const char* configure_name,
                              const char* launch_name, size_t lds, void** handle) {
  { const char* sw = getenv("MOOG_STEP_SPEC"); if (sw && atoi(sw) == 0) return nullptr; }   // 0: the generic kernels (A/B runs, tests)
  std::string dir;
  if (const char* d = getenv("MOOG_SPEC_DIR")) dir = d;
  else {
    Dl_info info;
    if (!dladdr(reinterpret_cast<const void*>(&moog_abi_version), &info) || !info.dli_fname) return nullptr;
    dir = info.dli_fname;
    const size_t cut = dir.find_last_of('/');
    dir = (cut == std::string::npos ? std::string(".") : dir.substr(0, cut)) + "/spec";
  }
  const bool full = e->maze_kernel && !e->late_reset;
  char name[96];
  snprintf(name, sizeof name, "/%s_%016llx_d%dw%d.so", prefix, (unsigned long long)program_hash(prog), full ? 2 : (e->dynamic_rules ? 1 : 0), e->step_wps);
  const std::string path = dir + name;
  if (access(path.c_str(), R_OK) != 0) return nullptr;
  void* h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
  if (!h) { fprintf(stderr, "moog: %s does not load (%s); the generic step kernel is used\n", path.c_str(), dlerror()); return nullptr; }
  typedef int (*fn_i)(void);
  typedef unsigned long long (*fn_u)(void);
  typedef const void* (*fn_p)(void);
  typedef int (*fn_cfg)(size_t);
  fn_i abi = reinterpret_cast<fn_i>(dlsym(h, "moog_spec_abi")), var = reinterpret_cast<fn_i>(dlsym(h, "moog_spec_variant"));
  fn_u hash = reinterpret_cast<fn_u>(dlsym(h, "moog_spec_hash")), ksz = reinterpret_cast<fn_u>(dlsym(h, "moog_spec_kargs_size"));
  fn_u dig = reinterpret_cast<fn_u>(dlsym(h, "moog_spec_source_digest"));
  // (the sources first: an object of another build of the same ABI number may differ in anything)
  if (!dig || dig() != MOOG_SRC_DIGEST || MOOG_SRC_DIGEST == 0ull) {
    fprintf(stderr, "moog: %s was built from other kernel sources or flags (digest %016llx, this library %016llx); the generic step "
            "kernel is used -- rebuild it (python -m moog._spec ..., __graft_entry__.build())\n", path.c_str(),
            dig ? dig() : 0ull, (unsigned long long)MOOG_SRC_DIGEST);
    dlclose(h);
    return nullptr;
  }
  fn_p pr = reinterpret_cast<fn_p>(dlsym(h, "moog_spec_program"));
  fn_cfg cfg = reinterpret_cast<fn_cfg>(dlsym(h, configure_name));
  void* launch = dlsym(h, launch_name);
  const bool ok = abi && var && hash && ksz && pr && cfg && launch && abi() == MOOG_ABI_VERSION && ksz() == sizeof(KArgs) &&
                  var() == ((full ? 2 : (e->dynamic_rules ? 1 : 0)) | (e->step_wps << 8)) && hash() == program_hash(prog) &&
                  memcmp(pr(), prog, sizeof(moog_program_t)) == 0 && cfg(lds) == (int)hipSuccess;
  if (!ok) {
    fprintf(stderr, "moog: %s was built for another program, variant or ABI; the generic step kernel is used\n", path.c_str());
    dlclose(h);
    return nullptr;
  }
  *handle = h;
  return launch;
}

static void load_spec_kernel(moog_engine* e, const moog_program_t* prog) {
  void* launch = load_spec_object(e, prog, "step", "moog_spec_configure", "moog_spec_launch", e->step_lds, &e->spec_handle);
  e->spec_launch = reinterpret_cast<void (*)(int, size_t, hipStream_t, const KArgs*)>(launch);
}

static void load_spec_plan_kernel(moog_engine* e, const moog_program_t* prog) {
  void* launch = load_spec_object(e, prog, "plan", "moog_spec_configure_3", "moog_spec_launch_3", e->plan_lds, &e->spec_plan_handle);
  e->spec_plan_launch = reinterpret_cast<void (*)(int, size_t, hipStream_t, const KArgs*)>(launch);
}
