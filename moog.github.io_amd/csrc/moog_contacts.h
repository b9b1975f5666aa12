// moog_contacts.h -- contacts observers (the Contacts observer; include/moog_engine.h moog_engine_add_contacts): the function
// one wavefront of the kernel of moog_contacts.hip runs per (env, observer), and the host code that turns a moog_contacts_t
// into the kernel's descriptors.  Everything here is host AND device code: tests/csrc/contacts_model.cpp compiles this header
// with g++ -O2 -ffp-contract=off and walks the same text lane by lane over host records (tests/test_contacts_host.py).
//
// What an entry says.  All arithmetic is fp64 without contraction.  For the ORDERED pair (a, b) = (row i of the first list, row
// j of the second) the entry is 1 iff
//   both slots are alive, they are different slots, both have opacity > 0 under MOOG_CONTACTS_VISIBLE_ONLY, and
//   sprite.py:462-484 overlaps_sprite(a, b) holds on the record as it stands:
//     circle.   dx = ax - bx, dy = ay - by over `position`; sqrt(fma(dy, dy, dx * dx)) > maxr_a + maxr_b gives 0 (numpy's 1-D
//               norm as the fixtures' numpy computes it).  A NaN fails the comparison and lets the pair through.
//     path.     Path.intersects_path(a, b, filled=True) as oracle/moog_oracle.c states it: with n = min(nverts, capacity)
//               vertices per polygon (n < 1: 0); a polygon without a finite vertex is an empty path and overlaps every polygon of
//               at least two vertices; else any pair of non-degenerate edges (squared length not isclose to 0) for which
//               matplotlib's segments_intersect holds; else every vertex of b inside a, or every vertex of a inside b, by the
//               even-odd point_in_path test.
//   The segment test's parallel branch measures from the first segment's end points, so the predicate is not symmetric in
//   general (moog_ct_seg_kind answers 1 and 4).
// No torus wrap-around and no polygon modifier: arena coordinates.
//
// Culls.  The circle test is the reference's own and is evaluated exactly as written above.  Every other cull rejects only what
// cannot be true: Path.intersects_path can only hold when the polygons come within matplotlib's isclose tolerances (rtol 1e-10,
// atol 1e-13) of each other, so two polygons, an edge and a polygon, or two edges that are more than MOOG_CT_MARGIN = 1e-5
// apart along an axis never meet (the argument of csrc/moog_device.h BB_MARGIN, for arena-sized coordinates).  Here the 8-DOPs
// (extents along x, y, x + y, x - y) are fp64 and built from the record's vertices, so no rounding of the box enters.  A row
// with ANY non-finite vertex gets a NaN box, which fails every comparison and never rejects.
//
// Symmetry.  When both lists are the same list the kernel evaluates (i, j) for i < j and fills (j, i) from it only where the
// narrow phase proves the answer symmetric the way the step kernel does (`proper`): true by a crossing of two non-parallel
// edges (kind 2: den, n1, n2 become -den, -n2, -n1 exactly with the segments exchanged), or false, or decided by the empty-path
// rule, without a parallel pair (kind 1 or 4) among the edge pairs tested -- the culls, the degenerate-edge skip and the two
// containment tests are symmetric in a and b as a set.  Otherwise it evaluates (j, i) as well.
//
// The mapping.  One wavefront -- a workgroup of 64 lanes -- per (env, observer); one launch serves every observer of the engine
// (grid x = env, y = observer).  The wave
//   1. builds per row, lanes = rows, in LDS: active (alive, visible), slot, vertex count, centre, max_radius, the 8-DOP and
//      "has a finite vertex"; clears the result bit set;
//   2. broad phase, lanes = pairs: the active rows of each list are compacted first, so only pairs of active rows are
//      enumerated (with one list, the pairs i < j: half of them); 64 pairs a pass are rejected by slot, circle and DOP;
//      survivors are compacted by ballot and prefix count into a candidate list in LDS of `chunk` entries; a full list is
//      drained, so LDS holds a chunk whatever R0 * R1 is;
//   3. narrow phase: a candidate gets a group of 16 lanes, four candidates at a time.  A group compacts the edges of each
//      polygon that reach the other's DOP (passes of 16 edges: a polygon has up to 128), enumerates the surviving edge pairs 16
//      at a time, stops at the first hit, and else runs the two containment tests with its lanes over vertices.  Vertices are
//      read from the record;
//   4. results go into the bit set through lane 0 (four at a time, in group order: no atomics, no two writers of a word);
//   5. expands the bit set to bytes: byte stores up to the first dword boundary of the env's block and behind the last, and
//      consecutive lanes writing consecutive dwords in between.  MOOG_CONTACTS_LAYER reduces the bits of a row's layer on the
//      fly, stopping at the first hit.
// The result is a pure function of the record: chunk size, grouping and drain order only decide when a bit is set.
//
// The host model needs the cross-lane steps too: as in moog_ray_sensor.h the wave function is written over the lane model of
// moog_wave_model.h.
#ifndef MOOG_CONTACTS_H_
#define MOOG_CONTACTS_H_

#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "moog_sprite_table.h"
#include "moog_wave_model.h"

#define MOOG_CT_GROUP 16                                   // lanes of one candidate pair in the narrow phase
#define MOOG_CT_GROUPS (MOOG_WAVE_LANES / MOOG_CT_GROUP)
#define MOOG_CT_CHUNK 256                                  // candidates held in LDS at a time
#define MOOG_CT_MAXV 128                                   // vertices of one polygon, at most (the engine's limit)
#define MOOG_CT_MARGIN 1e-5

// ---- descriptors -------------------------------------------------------------------------------------------------------
// One observer of a launch.  `rows` (device memory for the kernel): per row slot | layer id << 16, the slot's first vertex
// (program.slot_voff) and its vertex capacity (slot_vcap); the n0 rows of the first list, then -- unless `same` -- the n1 rows
// of the second.  The layer id of a second-list row is the position of its layer among that list's layers.
struct CtObs {
  uint8_t* out;   // [n_envs][n0][n1] (pair) or [n_envs][n0][n_layers1] (layer)
  const int32_t* rows;
  int32_t n0, n1, base1, n_layers1, flags, mode, same;
};
// The kernel's arguments, by value.
struct CtArgs {
  const double* f64;
  const int32_t* i32;
  int64_t f64_per_env, i32_per_env;
  int32_t n_envs, n_obs, chunk;   // chunk: 1 .. MOOG_CT_CHUNK (the kernel's launches use MOOG_CT_CHUNK)
  int32_t o_flags, o_nverts, o_opacity, o_pos, o_maxr, o_verts;
  CtObs c[MOOG_MAX_CONTACTS];
};
// A workgroup's LDS, carved out of one dynamic block: the arrays depend on the observer's row count.
struct CtLds {
  double *cx, *cy, *rad, *dop;   // [NR], [NR], [NR], [NR][8]: lo x, y, x+y, x-y, then hi
  int32_t* meta;                 // [NR]: active | finite << 1 | slot << 8 | n << 16
  uint32_t* bits;                // [ceil(n0 * n1 / 32)]
  uint32_t* cand;                // [MOOG_CT_CHUNK]: i << 16 | j
  int32_t* lstart;               // [MOOG_MAX_LAYERS + 2]: first second-list row of every layer of that list, then n1
  int32_t* gres;                 // [MOOG_CT_GROUPS]
  uint8_t* elist;                // [MOOG_CT_GROUPS][2][MOOG_CT_MAXV]
  uint8_t* alist;                // [2][MOOG_MAX_SLOTS]: the active rows of each list, ascending (rows of the second from 0)
};
MOOG_ST_HD int32_t moog_ct_rows(const CtObs& s) { return s.same ? s.n0 : s.n0 + s.n1; }
MOOG_ST_HD uint32_t moog_ct_words(const CtObs& s) { return ((uint32_t)s.n0 * (uint32_t)s.n1 + 31u) >> 5; }
MOOG_ST_HD size_t moog_ct_lds_bytes(const CtObs& s) {
  const size_t nr = (size_t)moog_ct_rows(s);
  return nr * 11 * sizeof(double) + nr * sizeof(int32_t) + moog_ct_words(s) * sizeof(uint32_t) + MOOG_CT_CHUNK * sizeof(uint32_t) +
         (MOOG_MAX_LAYERS + 2) * sizeof(int32_t) + MOOG_CT_GROUPS * sizeof(int32_t) + MOOG_CT_GROUPS * 2 * MOOG_CT_MAXV +
         2 * MOOG_MAX_SLOTS;
}
MOOG_ST_HD void moog_ct_carve(const CtObs& s, void* base, CtLds& l) {
  const size_t nr = (size_t)moog_ct_rows(s);
  l.cx = (double*)base; l.cy = l.cx + nr; l.rad = l.cy + nr; l.dop = l.rad + nr;
  l.meta = (int32_t*)(l.dop + 8 * nr);
  l.bits = (uint32_t*)(l.meta + nr);
  l.cand = l.bits + moog_ct_words(s);
  l.lstart = (int32_t*)(l.cand + MOOG_CT_CHUNK);
  l.gres = l.lstart + MOOG_MAX_LAYERS + 2;
  l.elist = (uint8_t*)(l.gres + MOOG_CT_GROUPS);
  l.alist = l.elist + MOOG_CT_GROUPS * 2 * MOOG_CT_MAXV;
}

// Fills `d` (everything but out / rows) and `rows` [3 * (n_rows_0 + n_rows_1)] from a description; returns NULL, or why the
// description is refused.
static inline const char* moog_ct_describe(const moog_program_t* P, const moog_layout_t* L, const moog_contacts_t* T, CtObs* d,
                                           int32_t* rows) {
  if (T->n_rows_0 < 1 || T->n_rows_0 > MOOG_MAX_SLOTS) return "contacts: n_rows_0 outside 1 .. MOOG_MAX_SLOTS";
  if (T->n_rows_1 < 1 || T->n_rows_1 > MOOG_MAX_SLOTS) return "contacts: n_rows_1 outside 1 .. MOOG_MAX_SLOTS";
  if (T->mode != MOOG_CONTACTS_PAIR && T->mode != MOOG_CONTACTS_LAYER) return "contacts: mode is neither MOOG_CONTACTS_PAIR nor MOOG_CONTACTS_LAYER";
  if (T->flags & ~MOOG_CONTACTS_VISIBLE_ONLY) return "contacts: unknown flag bits";
  int32_t same = T->n_rows_0 == T->n_rows_1;
  int32_t nl = 0;
  for (int list = 0; list < 2; ++list) {
    const int32_t* rs = list ? T->row_slot_1 : T->row_slot_0;
    const int32_t n = list ? T->n_rows_1 : T->n_rows_0;
    uint8_t seen[MOOG_MAX_SLOTS];
    memset(seen, 0, sizeof seen);
    int32_t id = -1;
    for (int r = 0; r < n; ++r) {
      const int32_t s = rs[r];
      if (s < 0 || s >= L->S) return "contacts: a row's slot is outside the layout (0 .. n_slots - 1)";
      if (seen[s]) return "contacts: a slot is named by two rows of one list";
      seen[s] = 1;
      if (P->slot_vcap[s] > MOOG_CT_MAXV) return "contacts: a slot's vertex capacity is above 128";
      if (r == 0 || P->slot_layer[s] != P->slot_layer[rs[r - 1]]) ++id;   // (rows come layer after layer)
      int32_t* w = rows + 3 * (list * T->n_rows_0 + r);
      w[0] = s | (id << 16);
      w[1] = P->slot_voff[s];
      w[2] = P->slot_vcap[s];
      if (list && same && s != T->row_slot_0[r]) same = 0;
    }
    if (list) nl = id + 1;
  }
  if (nl > MOOG_MAX_LAYERS) return "contacts: the second list's rows do not come layer after layer";
  d->n0 = T->n_rows_0; d->n1 = T->n_rows_1; d->same = same; d->base1 = same ? 0 : T->n_rows_0;
  d->n_layers1 = nl; d->flags = T->flags; d->mode = T->mode;
  return nullptr;
}

// Everything of `a` but the observers, from a layout.
static inline void moog_ct_args(const moog_layout_t* L, const double* f64, const int32_t* i32, int32_t n_envs, CtArgs* a) {
  memset(a, 0, sizeof *a);
  a->f64 = f64; a->i32 = i32; a->f64_per_env = L->f64_per_env; a->i32_per_env = L->i32_per_env;
  a->n_envs = n_envs; a->chunk = MOOG_CT_CHUNK;
  a->o_flags = L->o_flags; a->o_nverts = L->o_nverts; a->o_opacity = L->o_opacity;
  a->o_pos = L->o_pos; a->o_maxr = L->o_maxr; a->o_verts = L->o_verts;
}

// ---- matplotlib _path restatements (oracle/moog_oracle.c has the citations) ----------------------------------------------
MOOG_ST_HD bool moog_ct_finite(double x) { return fabs(x) <= DBL_MAX; }
MOOG_ST_HD bool moog_ct_isclose(double a, double b) {
  return fabs(a - b) <= fmax(1e-10 * fmax(fabs(a), fabs(b)), 1e-13);
}
// 0: no intersection, the segments are not parallel; 1: collinear segments that overlap; 2: a crossing of two non-parallel
// segments; 4: parallel segments, no intersection.  0 and 2 are the same with the segments exchanged, 1 and 4 need not be.
MOOG_ST_HD int moog_ct_seg_kind(double x1, double y1, double x2, double y2, double x3, double y3, double x4, double y4) {
  const double den = ((y4 - y3) * (x2 - x1)) - ((x4 - x3) * (y2 - y1));
  if (moog_ct_isclose(den, 0.0)) {
    const double t_area = (x2 * y3 - x3 * y2) - x1 * (y3 - y2) + y1 * (x3 - x2);
    if (moog_ct_isclose(t_area, 0.0)) {
      if (x1 == x2 && x2 == x3)
        return ((fmin(y1, y2) <= fmin(y3, y4) && fmin(y3, y4) <= fmax(y1, y2)) ||
                (fmin(y3, y4) <= fmin(y1, y2) && fmin(y1, y2) <= fmax(y3, y4))) ? 1 : 4;
      return ((fmin(x1, x2) <= fmin(x3, x4) && fmin(x3, x4) <= fmax(x1, x2)) ||
              (fmin(x3, x4) <= fmin(x1, x2) && fmin(x1, x2) <= fmax(x3, x4))) ? 1 : 4;
    }
    return 4;
  }
  const double n1 = ((x4 - x3) * (y1 - y3)) - ((y4 - y3) * (x1 - x3));
  const double n2 = ((x2 - x1) * (y1 - y3)) - ((y2 - y1) * (x1 - x3));
  const double u1 = n1 / den, u2 = n2 / den;
  return ((u1 > 0.0 || moog_ct_isclose(u1, 0.0)) && (u1 < 1.0 || moog_ct_isclose(u1, 1.0)) &&
          (u2 > 0.0 || moog_ct_isclose(u2, 0.0)) && (u2 < 1.0 || moog_ct_isclose(u2, 1.0))) ? 2 : 0;
}
// even-odd crossing test against one closed polygon of n vertices
MOOG_ST_HD bool moog_ct_point_in_poly(const double* v, int n, double tx, double ty) {
  if (!(moog_ct_finite(tx) && moog_ct_finite(ty))) return false;
  int inside = 0;
  double x0 = v[0], y0 = v[1];
  for (int i = 0; i < n; ++i) {
    const int j = (i + 1 == n) ? 0 : i + 1;
    const double x1 = v[2 * j], y1 = v[2 * j + 1];
    const int f0 = (y0 >= ty), f1 = (y1 >= ty);
    if (f0 != f1 && (((y1 - ty) * (x0 - x1) >= (x1 - tx) * (y0 - y1)) == (f1 != 0))) inside ^= 1;
    x0 = x1; y0 = y1;
  }
  return inside != 0;
}

// ---- culls (see the head of the file) ------------------------------------------------------------------------------------
MOOG_ST_HD bool moog_ct_dop_apart(const double* a, const double* b) {
  const double M = MOOG_CT_MARGIN;
  return (a[0] > b[4] + M) | (b[0] > a[4] + M) | (a[1] > b[5] + M) | (b[1] > a[5] + M) |
         (a[2] > b[6] + M) | (b[2] > a[6] + M) | (a[3] > b[7] + M) | (b[3] > a[7] + M);
}
MOOG_ST_HD bool moog_ct_seg_outside_dop(double x1, double y1, double x2, double y2, const double* d) {
  const double M = MOOG_CT_MARGIN;
  const double p1 = x1 + y1, p2 = x2 + y2, m1 = x1 - y1, m2 = x2 - y2;
  return ((x1 > d[4] + M) & (x2 > d[4] + M)) | ((x1 < d[0] - M) & (x2 < d[0] - M)) |
         ((y1 > d[5] + M) & (y2 > d[5] + M)) | ((y1 < d[1] - M) & (y2 < d[1] - M)) |
         ((p1 > d[6] + M) & (p2 > d[6] + M)) | ((p1 < d[2] - M) & (p2 < d[2] - M)) |
         ((m1 > d[7] + M) & (m2 > d[7] + M)) | ((m1 < d[3] - M) & (m2 < d[3] - M));
}
MOOG_ST_HD bool moog_ct_segs_apart(double x11, double y11, double x12, double y12, double x21, double y21, double x22, double y22) {
  const double M = MOOG_CT_MARGIN;
  return ((x11 > x21 + M) & (x11 > x22 + M) & (x12 > x21 + M) & (x12 > x22 + M)) |
         ((x21 > x11 + M) & (x21 > x12 + M) & (x22 > x11 + M) & (x22 > x12 + M)) |
         ((y11 > y21 + M) & (y11 > y22 + M) & (y12 > y21 + M) & (y12 > y22 + M)) |
         ((y21 > y11 + M) & (y21 > y12 + M) & (y22 > y11 + M) & (y22 > y12 + M));
}
// the axis-aligned box of `in` reaches beyond that of `out`: no vertex set of `in` lies wholly inside `out`
MOOG_ST_HD bool moog_ct_box_leaves(const double* in, const double* out) {
  const double M = MOOG_CT_MARGIN;
  return (in[0] < out[0] - M) | (in[1] < out[1] - M) | (in[4] > out[4] + M) | (in[5] > out[5] + M);
}

// ---- the per-lane pieces -----------------------------------------------------------------------------------------------
// Row r of the observer into LDS, from the env whose words are q / f.
MOOG_ST_HD void moog_ct_row(const CtArgs& a, const CtObs& s, const int32_t* q, const double* f, const CtLds& l, int32_t r) {
  const int32_t slot = s.rows[3 * r] & 0xffff;
  bool active = (q[a.o_flags + slot] & MOOG_F_ALIVE) != 0;
  if ((s.flags & MOOG_CONTACTS_VISIBLE_ONLY) && !(q[a.o_opacity + slot] > 0)) active = false;
  int32_t n = q[a.o_nverts + slot];
  const int32_t cap = s.rows[3 * r + 2];
  if (n > cap) n = cap;
  if (n < 0) n = 0;
  const double nan = (double)NAN;
  double lo0 = nan, lo1 = nan, lo2 = nan, lo3 = nan, hi0 = nan, hi1 = nan, hi2 = nan, hi3 = nan;
  bool any = false;
  if (active && n > 0) {
    const double* V = f + a.o_verts + 2 * (int64_t)s.rows[3 * r + 1];
    bool all = true;
    lo0 = lo1 = lo2 = lo3 = (double)INFINITY;
    hi0 = hi1 = hi2 = hi3 = -(double)INFINITY;
    for (int32_t k = 0; k < n; ++k) {
      const double x = V[2 * k], y = V[2 * k + 1], p = x + y, m = x - y;
      const bool fin = moog_ct_finite(x) && moog_ct_finite(y);
      any = any || fin;
      all = all && fin;
      lo0 = fmin(lo0, x); hi0 = fmax(hi0, x); lo1 = fmin(lo1, y); hi1 = fmax(hi1, y);
      lo2 = fmin(lo2, p); hi2 = fmax(hi2, p); lo3 = fmin(lo3, m); hi3 = fmax(hi3, m);
    }
    if (!all) lo0 = lo1 = lo2 = lo3 = hi0 = hi1 = hi2 = hi3 = nan;   // (never rejects)
  }
  l.cx[r] = f[a.o_pos + 2 * slot]; l.cy[r] = f[a.o_pos + 2 * slot + 1]; l.rad[r] = f[a.o_maxr + slot];
  double* d = l.dop + 8 * r;
  d[0] = lo0; d[1] = lo1; d[2] = lo2; d[3] = lo3; d[4] = hi0; d[5] = hi1; d[6] = hi2; d[7] = hi3;
  l.meta[r] = (active ? 1 : 0) | (any ? 2 : 0) | (slot << 8) | (n << 16);
}

// `sqrt(fma(dy, dy, dx * dx)) > r0 + r1`, exactly.  The square root is only taken when the squared distance is within 1e-9
// (relative) of the squared threshold, where its rounding could matter; elsewhere the comparison of squares decides
// identically (sqrt is monotone and correctly rounded; the roundings of d2 and r * r are seven orders below 1e-9).  A NaN
// fails both shortcuts and then the comparison itself: not apart.
MOOG_ST_HD bool moog_ct_circles_apart(double dx, double dy, double r) {
  const double d2 = fma(dy, dy, dx * dx), r2 = r * r;
  const bool far = (d2 > r2 * (1.0 + 1e-9)) & (r >= 0.0), near = d2 < r2 * (1.0 - 1e-9);
  if (far | near) return far;
  return sqrt(d2) > r;
}

// Is the ordered pair (active row i of the first list, active row j of the second) a candidate: different slots, circles not
// apart (the reference's test, exactly) and DOPs not apart.
MOOG_ST_HD bool moog_ct_broad(const CtObs& s, const CtLds& l, int32_t i, int32_t j) {
  const int32_t ri = i, rj = s.base1 + j;
  if (((l.meta[ri] >> 8) & 0xff) == ((l.meta[rj] >> 8) & 0xff)) return false;
  if (moog_ct_circles_apart(l.cx[ri] - l.cx[rj], l.cy[ri] - l.cy[rj], l.rad[ri] + l.rad[rj])) return false;
  return !moog_ct_dop_apart(l.dop + 8 * ri, l.dop + 8 * rj);
}

// Pair p of the n * (n - 1) / 2 pairs u < v of 0 .. n - 1, in row order: an estimate from the closed form (exact operands in
// float32: n <= 256), put right on the integers.
MOOG_ST_HD uint32_t moog_ct_tri(uint32_t i, uint32_t n) { return i * (2u * n - i - 1u) / 2u; }   // pairs before row i
MOOG_ST_HD void moog_ct_unrank(uint32_t p, uint32_t n, uint32_t& u, uint32_t& v) {
  const float b = (float)(2u * n - 1u);
  const float disc = b * b - 8.0f * (float)p;
  int32_t i = (int32_t)((b - sqrtf(disc > 0.0f ? disc : 0.0f)) * 0.5f);
  if (i < 0) i = 0;
  if (i > (int32_t)n - 2) i = (int32_t)n - 2;
  while (moog_ct_tri((uint32_t)i + 1u, n) <= p) ++i;
  while (moog_ct_tri((uint32_t)i, n) > p) --i;
  u = (uint32_t)i;
  v = u + 1u + (p - moog_ct_tri(u, n));
}

// The byte of output element k of the env: bit k of the set (pair), or "any bit of row i in layer l" (layer).
MOOG_ST_HD uint32_t moog_ct_element(const CtObs& s, const CtLds& l, uint32_t k) {
  if (s.mode == MOOG_CONTACTS_PAIR) return (l.bits[k >> 5] >> (k & 31u)) & 1u;
  const uint32_t i = k / (uint32_t)s.n_layers1, ly = k - i * (uint32_t)s.n_layers1;
  for (uint32_t b = i * (uint32_t)s.n1 + (uint32_t)l.lstart[ly], e = i * (uint32_t)s.n1 + (uint32_t)l.lstart[ly + 1]; b < e; ++b)
    if ((l.bits[b >> 5] >> (b & 31u)) & 1u) return 1u;
  return 0u;
}

// Output elements k .. k + 3 as the bytes of one dword (all four exist).
MOOG_ST_HD uint32_t moog_ct_four(const CtObs& s, const CtLds& l, uint32_t k) {
  if (s.mode == MOOG_CONTACTS_PAIR) {   // four bits of one or two words of the set
    const uint32_t w = k >> 5, sh = k & 31u;
    uint64_t x = l.bits[w];
    if (sh > 28u) x |= (uint64_t)l.bits[w + 1u] << 32;
    const uint32_t b = (uint32_t)(x >> sh);
    return (b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21);
  }
  return moog_ct_element(s, l, k) | (moog_ct_element(s, l, k + 1) << 8) | (moog_ct_element(s, l, k + 2) << 16) |
         (moog_ct_element(s, l, k + 3) << 24);
}

// ---- the wave function -------------------------------------------------------------------------------------------------
// the 16 bits of a ballot that belong to the group of `lane`
MOOG_ST_HD uint32_t moog_ct_gbits(uint64_t m, int lane) { return (uint32_t)(m >> (lane & ~(MOOG_CT_GROUP - 1))) & 0xffffu; }

// Narrow phase of up to four ordered pairs at once: the group of 16 lanes g = lane / 16 takes the pair (row ra of the first
// list, row rb of the second; both as LDS row indices) when act is set.  Every lane of a group holds the same act / ra / rb and
// leaves with the same res (0 / 1) and proper.  A group's lanes may differ only between two ballots.
MOOG_ST_HD void moog_ct_narrow(const CtArgs& a, const CtObs& s, const double* f, const CtLds& l, int tid, const int32_t* act,
                               const int32_t* ra, const int32_t* rb, int32_t* res, int32_t* proper) {
  int32_t live[MOOG_WAVE_NP], na[MOOG_WAVE_NP], nb[MOOG_WAVE_NP], ca[MOOG_WAVE_NP], cb[MOOG_WAVE_NP], par[MOOG_WAVE_NP];
  int32_t f1[MOOG_WAVE_NP], f2[MOOG_WAVE_NP], f3[MOOG_WAVE_NP];
  const double* va[MOOG_WAVE_NP];
  const double* vb[MOOG_WAVE_NP];
  // the empty-path rule; a polygon without a vertex
  MOOG_WAVE_EACH_LANE {
    const int P = MOOG_WAVE_P;
    res[P] = 0; proper[P] = 1; par[P] = 0; ca[P] = cb[P] = 0; na[P] = nb[P] = 0; va[P] = vb[P] = f;
    live[P] = act[P];
    if (act[P]) {
      const int32_t ma = l.meta[ra[P]], mb = l.meta[rb[P]];
      na[P] = ma >> 16; nb[P] = mb >> 16;
      va[P] = f + a.o_verts + 2 * (int64_t)s.rows[3 * ra[P] + 1];
      vb[P] = f + a.o_verts + 2 * (int64_t)s.rows[3 * rb[P] + 1];
      const bool fa = (ma & 2) != 0, fb = (mb & 2) != 0;
      if (na[P] < 1 || nb[P] < 1) live[P] = 0;
      else if (!fa || !fb) {
        res[P] = (na[P] + 1 >= 3 && !fb) || (nb[P] + 1 >= 3 && !fa);
        live[P] = 0;
      }
    }
  }
  // the edges of a that reach b's DOP, and those of b that reach a's, compacted per group: 16 edges of each a pass
  for (int32_t k0 = 0; k0 < MOOG_CT_MAXV; k0 += MOOG_CT_GROUP) {
    MOOG_WAVE_EACH_LANE {
      const int P = MOOG_WAVE_P;
      const int32_t k = k0 + (lane & (MOOG_CT_GROUP - 1));
      f1[P] = f2[P] = 0;
      f3[P] = live[P] && (k0 < na[P] || k0 < nb[P]);
      if (live[P] && k < na[P]) {
        const int32_t k2 = (k + 1 == na[P]) ? 0 : k + 1;
        const double* v = va[P];
        f1[P] = !moog_ct_seg_outside_dop(v[2 * k], v[2 * k + 1], v[2 * k2], v[2 * k2 + 1], l.dop + 8 * rb[P]);
      }
      if (live[P] && k < nb[P]) {
        const int32_t k2 = (k + 1 == nb[P]) ? 0 : k + 1;
        const double* v = vb[P];
        f2[P] = !moog_ct_seg_outside_dop(v[2 * k], v[2 * k + 1], v[2 * k2], v[2 * k2 + 1], l.dop + 8 * ra[P]);
      }
    }
    if (MOOG_WAVE_BALLOT(f3) == 0) break;
    const uint64_t m1 = MOOG_WAVE_BALLOT(f1), m2 = MOOG_WAVE_BALLOT(f2);
    MOOG_WAVE_EACH_LANE {
      const int P = MOOG_WAVE_P;
      const int g = lane / MOOG_CT_GROUP, t = lane & (MOOG_CT_GROUP - 1);
      const uint32_t g1 = moog_ct_gbits(m1, lane), g2 = moog_ct_gbits(m2, lane), below = (1u << t) - 1u;
      uint8_t* el = l.elist + g * 2 * MOOG_CT_MAXV;
      if (f1[P]) el[ca[P] + MOOG_WAVE_POPC(g1 & below)] = (uint8_t)(k0 + t);
      if (f2[P]) el[MOOG_CT_MAXV + cb[P] + MOOG_WAVE_POPC(g2 & below)] = (uint8_t)(k0 + t);
      ca[P] += MOOG_WAVE_POPC(g1); cb[P] += MOOG_WAVE_POPC(g2);
    }
  }
  MOOG_WAVE_SYNC();
  // the surviving edge pairs, 16 of a group at a time, until a hit
  for (int32_t base = 0;; base += MOOG_CT_GROUP) {
    MOOG_WAVE_EACH_LANE {
      const int P = MOOG_WAVE_P;
      const int g = lane / MOOG_CT_GROUP;
      const int32_t idx = base + (lane & (MOOG_CT_GROUP - 1)), total = ca[P] * cb[P];
      f1[P] = f2[P] = 0;
      f3[P] = live[P] && base < total;
      int kind = 0;
      if (live[P] && idx < total) {
        const uint8_t* el = l.elist + g * 2 * MOOG_CT_MAXV;
        const int32_t ia = idx / cb[P], ib = idx - ia * cb[P];
        const int32_t i = el[ia], j = el[MOOG_CT_MAXV + ib];
        const int32_t i2 = (i + 1 == na[P]) ? 0 : i + 1, j2 = (j + 1 == nb[P]) ? 0 : j + 1;
        const double* v = va[P];
        const double* w = vb[P];
        const double x11 = v[2 * i], y11 = v[2 * i + 1], x12 = v[2 * i2], y12 = v[2 * i2 + 1];
        const double x21 = w[2 * j], y21 = w[2 * j + 1], x22 = w[2 * j2], y22 = w[2 * j2 + 1];
        if (!moog_ct_segs_apart(x11, y11, x12, y12, x21, y21, x22, y22)) {
          const bool dega = moog_ct_isclose((x11 - x12) * (x11 - x12) + (y11 - y12) * (y11 - y12), 0.0);
          const bool degb = moog_ct_isclose((x21 - x22) * (x21 - x22) + (y21 - y22) * (y21 - y22), 0.0);
          if (!dega && !degb) kind = moog_ct_seg_kind(x11, y11, x12, y12, x21, y21, x22, y22);
        }
      }
      f1[P] = (kind & 3) != 0;
      f2[P] = kind == 2;
      if (kind == 4) par[P] = 1;
    }
    if (MOOG_WAVE_BALLOT(f3) == 0) break;
    const uint64_t m1 = MOOG_WAVE_BALLOT(f1), m2 = MOOG_WAVE_BALLOT(f2);
    MOOG_WAVE_EACH_LANE {
      const int P = MOOG_WAVE_P;
      if (live[P] && moog_ct_gbits(m1, lane)) {
        res[P] = 1; proper[P] = moog_ct_gbits(m2, lane) != 0; live[P] = 0;
      }
    }
  }
  {
    const uint64_t mp = MOOG_WAVE_BALLOT(par);
    MOOG_WAVE_EACH_LANE par[MOOG_WAVE_P] = moog_ct_gbits(mp, lane) != 0;
  }
  // path_in_path both ways: every vertex of one inside the other (possible only when its box does not leave the other's)
  for (int way = 0; way < 2; ++way) {
    MOOG_WAVE_EACH_LANE {
      const int P = MOOG_WAVE_P;
      const int32_t no = way ? nb[P] : na[P], ni = way ? na[P] : nb[P];   // outer and inner polygon
      const double* vo = way ? vb[P] : va[P];
      const double* vi = way ? va[P] : vb[P];
      const int32_t ro = way ? rb[P] : ra[P], ri = way ? ra[P] : rb[P];
      f1[P] = f2[P] = 0;
      if (live[P] && no + 1 >= 3 && ni > 0 && !moog_ct_box_leaves(l.dop + 8 * ri, l.dop + 8 * ro)) {
        f1[P] = 1;
        for (int32_t k = lane & (MOOG_CT_GROUP - 1); k < ni && !f2[P]; k += MOOG_CT_GROUP)
          f2[P] = !moog_ct_point_in_poly(vo, no, vi[2 * k], vi[2 * k + 1]);
      }
    }
    const uint64_t m2 = MOOG_WAVE_BALLOT(f2);
    MOOG_WAVE_EACH_LANE {
      const int P = MOOG_WAVE_P;
      if (f1[P] && !moog_ct_gbits(m2, lane)) { res[P] = 1; proper[P] = 0; live[P] = 0; }
    }
  }
  MOOG_WAVE_EACH_LANE {
    const int P = MOOG_WAVE_P;
    if (live[P]) { res[P] = 0; proper[P] = !par[P]; }
  }
}

// The first nc candidates of the list, four at a time.
MOOG_ST_HD void moog_ct_drain(const CtArgs& a, const CtObs& s, const double* f, const CtLds& l, int tid, int32_t nc) {
  int32_t act[MOOG_WAVE_NP], ra[MOOG_WAVE_NP], rb[MOOG_WAVE_NP], res[MOOG_WAVE_NP], proper[MOOG_WAVE_NP];
  int32_t act2[MOOG_WAVE_NP], res2[MOOG_WAVE_NP], proper2[MOOG_WAVE_NP];
  for (int32_t c0 = 0; c0 < nc; c0 += MOOG_CT_GROUPS) {
    MOOG_WAVE_EACH_LANE {
      const int P = MOOG_WAVE_P;
      const int32_t c = c0 + lane / MOOG_CT_GROUP;
      act[P] = c < nc;
      const uint32_t pr = act[P] ? l.cand[c] : 0u;
      ra[P] = (int32_t)(pr >> 16); rb[P] = s.base1 + (int32_t)(pr & 0xffffu);
    }
    moog_ct_narrow(a, s, f, l, tid, act, ra, rb, res, proper);
    MOOG_WAVE_EACH_LANE { const int P = MOOG_WAVE_P; act2[P] = act[P] && s.same && !proper[P]; res2[P] = res[P]; }
    if (s.same && MOOG_WAVE_BALLOT(act2) != 0) {   // (j, i) on its own where (i, j) does not prove it
      MOOG_WAVE_SYNC();
      moog_ct_narrow(a, s, f, l, tid, act2, rb, ra, res2, proper2);
      MOOG_WAVE_EACH_LANE { const int P = MOOG_WAVE_P; if (!act2[P]) res2[P] = res[P]; }
    }
    MOOG_WAVE_EACH_LANE {
      const int P = MOOG_WAVE_P;
      if ((lane & (MOOG_CT_GROUP - 1)) == 0) l.gres[lane / MOOG_CT_GROUP] = act[P] ? (res[P] | (res2[P] << 1)) : 0;
    }
    MOOG_WAVE_SYNC();
    MOOG_WAVE_EACH_LANE {
      if (lane == 0)
        for (int g = 0; g < MOOG_CT_GROUPS && c0 + g < nc; ++g) {
          const uint32_t pr = l.cand[c0 + g], i = pr >> 16, j = pr & 0xffffu;
          const int32_t r = l.gres[g];
          if (r & 1) { const uint32_t k = i * (uint32_t)s.n1 + j; l.bits[k >> 5] |= 1u << (k & 31u); }
          if (s.same && (r & 2)) { const uint32_t k = j * (uint32_t)s.n1 + i; l.bits[k >> 5] |= 1u << (k & 31u); }
        }
    }
    MOOG_WAVE_SYNC();
  }
}

// Observer s of env `env`, by one wave: tid is the thread's lane on the device and unused on the host, where one call runs
// all 64 lanes.  `lds_base`: moog_ct_lds_bytes(s) bytes, 8-byte aligned.  Returns the candidates past the broad phase.
MOOG_ST_HD int32_t moog_ct_wave(const CtArgs& a, const CtObs& s, int64_t env, void* lds_base, int tid) {
  const int32_t* q = a.i32 + env * a.i32_per_env;
  const double* f = a.f64 + env * a.f64_per_env;
  CtLds l;
  moog_ct_carve(s, lds_base, l);
  const int32_t NR = moog_ct_rows(s);
  const uint32_t NW = moog_ct_words(s);
  MOOG_WAVE_EACH_LANE {
    for (int32_t r = lane; r < NR; r += MOOG_WAVE_LANES) moog_ct_row(a, s, q, f, l, r);
    for (uint32_t w = (uint32_t)lane; w < NW; w += MOOG_WAVE_LANES) l.bits[w] = 0u;
    for (int32_t j = lane; j < s.n1; j += MOOG_WAVE_LANES) {
      const int32_t id = s.rows[3 * (s.base1 + j)] >> 16;
      if (j == 0 || id != (s.rows[3 * (s.base1 + j - 1)] >> 16)) l.lstart[id] = j;
      if (j == s.n1 - 1) l.lstart[id + 1] = s.n1;
    }
  }
  MOOG_WAVE_SYNC();
  int32_t keep[MOOG_WAVE_NP];
  uint32_t pair[MOOG_WAVE_NP];
  // the active rows of each list, compacted in row order: the broad phase enumerates pairs of active rows only
  uint32_t A0 = 0, A1 = 0;
  const uint8_t* alist1 = s.same ? l.alist : l.alist + MOOG_MAX_SLOTS;
  for (int list = 0; list < (s.same ? 1 : 2); ++list) {
    const int32_t n = list ? s.n1 : s.n0, base = list ? s.base1 : 0;
    uint32_t cnt = 0;
    for (int32_t r0 = 0; r0 < n; r0 += MOOG_WAVE_LANES) {
      MOOG_WAVE_EACH_LANE keep[MOOG_WAVE_P] = r0 + lane < n && (l.meta[base + r0 + lane] & 1);
      const uint64_t m = MOOG_WAVE_BALLOT(keep);
      MOOG_WAVE_EACH_LANE
        if (keep[MOOG_WAVE_P]) l.alist[list * MOOG_MAX_SLOTS + cnt + MOOG_WAVE_POPC(m & ((1ull << lane) - 1ull))] = (uint8_t)(r0 + lane);
      cnt += (uint32_t)MOOG_WAVE_POPC(m);
    }
    if (list) A1 = cnt; else A0 = cnt;
  }
  if (s.same) A1 = A0;
  MOOG_WAVE_SYNC();
  // broad phase: 64 pairs a pass -- with `same` the pairs i < j only; survivors are appended to the candidate list, which is
  // drained whenever it is full
  const uint32_t NP = (uint32_t)s.n0 * (uint32_t)s.n1;
  const uint32_t NB = s.same ? A0 * (A0 - (A0 ? 1u : 0u)) / 2u : A0 * A1;
  int32_t ncand = 0, seen = 0;
  for (uint32_t p0 = 0; p0 < NB; p0 += MOOG_WAVE_LANES) {
    MOOG_WAVE_EACH_LANE {
      const int P = MOOG_WAVE_P;
      const uint32_t p = p0 + (uint32_t)lane;
      keep[P] = 0; pair[P] = 0;
      if (p < NB) {
        uint32_t u, v;
        if (s.same) moog_ct_unrank(p, A0, u, v);
        else { u = p / A1; v = p - u * A1; }
        const uint32_t i = l.alist[u], j = alist1[v];
        keep[P] = moog_ct_broad(s, l, (int32_t)i, (int32_t)j);
        pair[P] = (i << 16) | j;
      }
    }
    const uint64_t m = MOOG_WAVE_BALLOT(keep);
    const int32_t total = MOOG_WAVE_POPC(m);
    seen += total;
    for (int32_t done = 0; done < total;) {
      const int32_t room = a.chunk - ncand, take = total - done < room ? total - done : room;
      MOOG_WAVE_EACH_LANE {
        const int P = MOOG_WAVE_P;
        const int32_t rank = MOOG_WAVE_POPC(m & ((1ull << lane) - 1ull));
        if (keep[P] && rank >= done && rank < done + take) l.cand[ncand + rank - done] = pair[P];
      }
      ncand += take; done += take;
      if (ncand == a.chunk) {
        MOOG_WAVE_SYNC();
        moog_ct_drain(a, s, f, l, tid, ncand);
        ncand = 0;
      }
    }
  }
  MOOG_WAVE_SYNC();
  if (ncand) moog_ct_drain(a, s, f, l, tid, ncand);
  MOOG_WAVE_SYNC();
  // the env's block of bytes: byte stores up to the first dword boundary and behind the last, dword stores in between
  const uint32_t NE = s.mode == MOOG_CONTACTS_PAIR ? NP : (uint32_t)s.n0 * (uint32_t)s.n_layers1;
  uint8_t* out = s.out + env * (int64_t)NE;
  uint32_t head = (uint32_t)((4u - ((uintptr_t)out & 3u)) & 3u);
  if (head > NE) head = NE;
  const uint32_t nd = (NE - head) >> 2, tail0 = head + 4u * nd;
  MOOG_WAVE_EACH_LANE {
    if ((uint32_t)lane < head) out[lane] = (uint8_t)moog_ct_element(s, l, (uint32_t)lane);
    for (uint32_t d = (uint32_t)lane; d < nd; d += MOOG_WAVE_LANES) {
      const uint32_t k = head + 4u * d;
      *(uint32_t*)(out + k) = moog_ct_four(s, l, k);
    }
    if (tail0 + (uint32_t)lane < NE) out[tail0 + lane] = (uint8_t)moog_ct_element(s, l, tail0 + (uint32_t)lane);
  }
  return seen;
}

#if defined(__HIPCC__)
void moog_contacts_launch(CtArgs a, hipStream_t stream);   // moog_contacts.hip
#endif

#endif  // MOOG_CONTACTS_H_
