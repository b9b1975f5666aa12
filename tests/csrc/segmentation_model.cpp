// Host model of the segmentation views (moog_engine_add_segmentation): the emitter with the ids as its per-slot colours, the
// mask rasteriser's phases through p4 and rm_p5_ids (moog.github.io_amd/csrc/moog_raster_mask_core.h), run thread by thread
// on the CPU with the barriers as loop boundaries -- what moog_raster_ids_kernel runs.  Test infrastructure
// (tests/test_segmentation_model.py), beside raster_mask_model.cpp, which models the frames' kernel.
#include <stdlib.h>
#include <vector>

#include "../../moog.github.io_amd/csrc/moog_raster_mask_core.h"

// what the row masks of the pass in hand say: the last item (painter's order = item order) with opacity != 0 whose mask covers a pixel
template <int WORDS>
static void expect_from_masks(const RmArgs& a, const RmCtx& c, int base, int end, uint8_t* want) {
  for (int g = base; g < end; ++g) {
    const RmItem it = c.info[g];
    int ys;
    const int cnt = rm_item_rows(a, c, g, 0, &ys);
    if ((it.rgba >> 24) == 0u) continue;
    for (int y = ys; y < ys + cnt; ++y) {
      const uint64_t* m = reinterpret_cast<const uint64_t*>(c.rows + it.rowbase + y);
      for (int x = 0; x < a.W; ++x)
        if ((m[WORDS > 1 ? (x >> 6) : 0] >> (x & 63)) & 1ull) want[(size_t)(a.flip ? a.H - 1 - y : y) * a.W + x] = (uint8_t)(it.rgba & 0xffu);
    }
  }
}

// load .. p5 of one frame whose draw record is in place; want (or null): [H][W], zeroed by the caller
template <int WORDS, bool COMPACT>
static int model_frame(const RmArgs& a, const RmCtx& c, int env, int T, uint8_t* want) {
  const int waves = T / 64;
  int passes = 0;
  for (int t = 0; t < T; ++t) rm_load(a, c, env, t, T);
  for (int base = 0;;) {
    const int end = rm_pass_end(a, c, base);
    const int total_rows = c.rowoff[end] - c.rowoff[base];
    if (!c.misc[6]) for (int w = 0; w < waves; ++w) rm_p2_assign(a, c, base, end, 0, -1);
    for (int t = 0; t < T; ++t) rm_p3<WORDS, COMPACT>(a, c, base, end, 0, t, T);
    { RmSortKey sk; for (int t = 0; t < T; ++t) rm_p4a(c, total_rows, t, T, sk); for (int t = 0; t < T; ++t) rm_p4b(c, total_rows, t, T, sk); }
    for (int t = 0; t < T; ++t) rm_p4<WORDS, COMPACT>(a, c, total_rows, t, T, c.xx + (t / 64) * a.plan.xx_stride);
    if (a.big) for (int t = 0; t < T; ++t) rm_p4_big<WORDS, COMPACT>(a, c, t, T, c.xx + (t / 64) * a.plan.xx_stride, reinterpret_cast<uint8_t*>(c.xx + waves * a.plan.xx_stride));
    if (want) expect_from_masks<WORDS>(a, c, base, end, want);
    for (int t = 0; t < T; ++t) rm_p5_ids<WORDS>(a, c, env, base == 0, t, T);
    ++passes;
    if (end >= a.S) break;
    base = end;
    for (int t = 0; t < T; ++t) rm_next_pass(a, c, t, T);
  }
  return passes;
}

static int run_frame(const RmArgs& a, const RmCtx& c, int env, int T, uint8_t* want) {
  if (a.W > 64) return a.compact ? model_frame<2, true>(a, c, env, T, want) : model_frame<2, false>(a, c, env, T, want);
  return a.compact ? model_frame<1, true>(a, c, env, T, want) : model_frame<1, false>(a, c, env, T, want);
}

extern "C" {

// The id images of n_envs state records under a segmentation; ids: [n_envs][H][Wpad] (Wpad = width rounded up to 16).
// stats: [0] passes.  Returns 0, or < 0 for a frame the mask rasteriser does not take.
int seg_model_frames(const moog_program_t* P, const moog_segmentation_t* G, const double* f64, const int32_t* i32, int n_envs,
                     uint8_t* ids, int threads, int cap_rows, int compact, long long* stats) {
  moog_layout_t L;
  moog_layout(P, &L);
  RmArgs a;
  memset(&a, 0, sizeof a);
  RmEmit em;
  memset(&em, 0, sizeof em);
  a.image = ids;
  for (int sl = 0; sl < P->n_slots; ++sl) {
    if (P->slot_vcap[sl] > RM_BIG_NV) return -2;
    if (P->slot_vcap[sl] > RM_MAX_NV) a.big = 1;
  }
  em.ncopy = G->polymod == MOOG_POLYMOD_TORUS ? 9 : 1;
  a.n_envs = n_envs; em.slots = P->n_slots; em.S = a.S = P->n_slots * em.ncopy;
  if (a.S > 256 || G->n_slots != P->n_slots) return -4;
  a.W = (G->width + 15) & ~15; a.H = G->height; a.flip = 1;
  em.W = a.W; em.H = a.H; em.scale_w = G->width;
  if (a.W > 128 || a.H > 128) return -3;
  a.cap_rows = cap_rows < a.H ? a.H : cap_rows;
  a.iwords = (a.S + 31) / 32;
  em.cmap = MOOG_CMAP_IDENTITY;
  em.first_person = G->polymod == MOOG_POLYMOD_FIRST_PERSON;
  if (em.first_person) { em.fp_slot0 = P->layer_slot0[G->polymod_layer]; em.fp_nslots = P->layer_nslots[G->polymod_layer]; }
  a.threads = threads;
  std::vector<uint32_t> id_words((size_t)n_envs * P->n_slots);   // the engine's per-env copy of slot_id
  for (int env = 0; env < n_envs; ++env)
    for (int sl = 0; sl < P->n_slots; ++sl) id_words[(size_t)env * P->n_slots + sl] = G->slot_id[sl];
  em.rgb_override = id_words.data();
  em.lay = rm_draw_layout(em.S, L.TOTV * em.ncopy);
  std::vector<uint8_t> draw((size_t)n_envs * em.lay.stride, 0xCD);
  em.out = draw.data();
  a.draw = draw.data(); a.lay = em.lay;
  const int T = threads, waves = T / 64;
  a.compact = compact;
  rm_plan(a.S, L.TOTV * em.ncopy, a.W, a.H, a.cap_rows, a.iwords, waves, a.big, &a.plan, compact);
  std::vector<unsigned char> lds(a.plan.total + 64);
  const RmCtx c = rm_ctx(a.plan, lds.data());
  std::vector<uint32_t> vinfo((size_t)(L.TOTV > 0 ? L.TOTV : 1), 0u);
  for (int sl = 0; sl < P->n_slots; ++sl)
    for (int k = 0; k < P->slot_vcap[sl]; ++k) vinfo[P->slot_voff[sl] + k] = (uint32_t)sl | ((uint32_t)k << 8);
  std::vector<long long> scratch((RM_EMIT_SCRATCH_WORDS(em.slots, em.S, em.ncopy) + 1) / 2);
  for (int env = 0; env < n_envs; ++env) {
    RmSrcRecord src;
    src.P = P; src.L = &L; src.f = f64 + (size_t)env * L.f64_per_env; src.q = i32 + (size_t)env * L.i32_per_env; src.vi = vinfo.data();
    for (auto& w : scratch) w = (long long)0xA5A5A5A5A5A5A5A5ull;   // (whatever the LDS held)
    RmEmitScratch sc;
    rm_emit_scratch(reinterpret_cast<int32_t*>(scratch.data()), em.slots, em.ncopy, &sc);
    rm_emit(em, src, env, -1, sc, L.TOTV);
    memset(lds.data(), 0xA5, lds.size());   // LDS is not zero when a workgroup starts
    const int passes = run_frame(a, c, env, T, nullptr);
    if (stats) stats[0] += passes;
  }
  return 0;
}

// One frame of n_poly polygons given as integer canvas points (xy: their points one after the other, nv[k] <= RM_MAX_NV each)
// with an id and an opacity each, on a W x H canvas (W a multiple of 16): `got` = what rm_p5_ids composes, `want` = the last
// polygon with opacity != 0 whose coverage mask -- the row masks p4 left, the ones the frames' compose reads -- has the
// pixel's bit.  Both [H][W], zeroed here.  Returns the number of passes, or < 0.
int seg_model_polygons(const int* xy, const int* nv, const uint8_t* id, const uint8_t* alpha, int n_poly, int W, int H,
                       int cap_rows, int compact, uint8_t* got, uint8_t* want) {
  if (n_poly < 1 || n_poly > 256 || (W & 15) || W > 128 || H > 128) return -1;
  int n_pts = 0;
  for (int k = 0; k < n_poly; ++k) { if (nv[k] < 0 || nv[k] > RM_MAX_NV) return -2; n_pts += nv[k]; }
  RmArgs a;
  memset(&a, 0, sizeof a);
  a.n_envs = 1; a.S = n_poly; a.W = W; a.H = H; a.flip = 1; a.iwords = (n_poly + 31) / 32; a.threads = RM_THREADS;
  a.cap_rows = cap_rows < H ? H : cap_rows;
  a.compact = compact;
  a.lay = rm_draw_layout(n_poly, n_pts > 0 ? n_pts : 1);
  std::vector<uint8_t> draw(a.lay.stride, 0xCD);
  RmDrawItem* items = reinterpret_cast<RmDrawItem*>(draw.data() + a.lay.o_items);
  uint32_t* pts = reinterpret_cast<uint32_t*>(draw.data() + a.lay.o_pts);
  uint8_t* owner = draw.data() + a.lay.o_owner;
  int first = 0, rows = 0;
  for (int k = 0; k < n_poly; ++k) {   // the record as the emitter writes it (moog_draw_record.h)
    int ymin = 32767, ymax = -32768;
    for (int j = 0; j < nv[k]; ++j) {
      const int x = rm_clamp16(xy[2 * (first + j)]), y = rm_clamp16(xy[2 * (first + j) + 1]);
      pts[first + j] = (uint32_t)(uint16_t)x | ((uint32_t)(uint16_t)y << 16);
      owner[first + j] = (uint8_t)k;
      if (y < ymin) ymin = y;
      if (y > ymax) ymax = y;
    }
    RmDrawItem o;
    o.rowoff = rows;
    o.pb_nv = (uint32_t)first | ((uint32_t)nv[k] << 20);
    o.y01 = nv[k] > 0 ? (int32_t)((uint32_t)(uint16_t)ymin | ((uint32_t)(uint16_t)ymax << 16)) : RM_Y01_EMPTY;
    o.rgba = nv[k] > 0 ? ((uint32_t)id[k] | ((uint32_t)alpha[k] << 24)) : 0u;
    items[k] = o;
    rows += nv[k] > 0 ? rm_rows_on_canvas(ymin, ymax, H) : 0;
    first += nv[k];
  }
  RmDrawHdr h;
  h.n_pts = n_pts; h.total_rows = rows; h.flags = 0; h.pad = 0;
  *reinterpret_cast<RmDrawHdr*>(draw.data()) = h;
  a.draw = draw.data();
  memset(got, 0, (size_t)W * H);
  memset(want, 0, (size_t)W * H);
  a.image = got;
  rm_plan(a.S, n_pts > 0 ? n_pts : 1, W, H, a.cap_rows, a.iwords, RM_THREADS / 64, 0, &a.plan, compact);
  std::vector<unsigned char> lds(a.plan.total + 64, 0xA5);
  const RmCtx c = rm_ctx(a.plan, lds.data());
  return run_frame(a, c, 0, RM_THREADS, want);
}

// csrc/moog_raster_mask_core.h rm_plan's total for a frame of `items` polygons and `points` points (two wavefronts): what
// moog._compiler.mask_plan_bytes restates
long long seg_model_plan_bytes(int items, int points, int W, int H, int cap_rows, int big, int compact) {
  RmPlan plan;
  rm_plan(items, points, W, H, cap_rows, (items + 31) / 32, RM_THREADS / 64, big, &plan, compact);
  return (long long)plan.total;
}

}  // extern "C"
