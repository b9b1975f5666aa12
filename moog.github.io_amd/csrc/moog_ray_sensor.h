// moog_ray_sensor.h -- ray sensors (the RaySensor observer; include/moog_engine.h moog_engine_add_sensor): the function one
// wavefront of the kernel of moog_ray_sensor.hip runs per (env, sensor), and the host code that turns a moog_sensor_t into
// the kernel's descriptors.  Everything here is host AND device code: tests/csrc/ray_sensor_model.cpp compiles this header
// with g++ -O2 -ffp-contract=off and walks the same text lane by lane over host records (tests/test_ray_sensor_host.py).
//
// What a sensor reads.  All arithmetic is fp64 without contraction, and every comparison is written so that a NaN operand
// fails it.
//   Origin.      O is `position` of the origin slot.  If that slot is not alive, every ray reads (max_range, 0).
//   Directions.  The caller computes them in float64 and hands them over as data: theta_k = heading + fov * ((k + 0.5) /
//                num_rays - 0.5), d_k = (cos theta_k, sin theta_k).
//   Rotation.    With MOOG_SENSOR_FOLLOW_ANGLE the device rotates d_k by the origin sprite's `angle`:
//                D = (c*dx - s*dy, s*dx + c*dy), with c, s the device's cos / sin.  Without it, D = d_k and the device does no
//                trigonometry.
//   Targets.     Targets are the rows' slots that are alive, are not the origin slot, and have opacity > 0 when
//                MOOG_SENSOR_VISIBLE_ONLY is set.  A target with n >= 2 vertices has edges v -> (v + 1) % n.
//   Ray against edge.  For edge A -> B, let E = B - A and W = A - O.  Then
//                den = Dx*Ey - Dy*Ex,  nt = Wx*Ey - Wy*Ex,  nu = Wx*Dy - Wy*Dx.
//                den == 0 (or not finite) is no hit.  Otherwise let sg be the sign of den.  The edge is hit iff sg*nt >= 0 and
//                0 <= sg*nu <= sg*den.  Both edge ends are inclusive, so nothing leaks through a vertex.
//                The hit distance is t = nt / den, one correctly rounded division, only for hits.  The hit is kept iff
//                t <= max_range.
//   Result per ray.  The smallest t wins.  Equal t resolves to the lowest row.  No hit reads (max_range, 0).
//   Cast.        t is cast to the output dtype once, round-to-nearest-even, with moog_st_round_bits (a winning -0.0 reads
//                +0.0).  Ids are exact in both dtypes.
//   Geometry not handled.  No torus wrap-around and no polygon modifier.  Rays run in arena coordinates over the record's
//                vertices.
//
// The mapping.  One wavefront -- a workgroup of 64 lanes -- per (env, sensor); one launch serves every sensor of the engine
// (grid x = env, y = sensor).  The wave
//   1. takes cos / sin of the origin's angle ONCE (lane 0, through LDS), only with MOOG_SENSOR_FOLLOW_ANGLE;
//   2. counts every row's edges (4 rows a lane; 0 for a row that is no target) and prefix-sums the counts over the wave with
//      shuffles, which numbers the env's edges 0 .. N - 1 in row order (RsLds::estart);
//   3. stages the edges through LDS in chunks of MOOG_RS_CHUNK, each as W = A - O, E = B - A (32 bytes, so that a lane reads
//      an edge with two 16-byte LDS reads: at the one or two waves per SIMD a small batch gives, 16-byte reads keep their rate
//      where 8-byte ones lose most of it) and a key, row | id << 16.  An env's edge count is bounded only by the record, so
//      LDS holds a chunk, never the env: 7.6 KB per workgroup whatever the capacities are.  A lane finds the row of edge e by
//      bisection over estart;
//   4. spreads its lanes over (ray, edge subset): G = the largest power of two with G * n_rays <= 64 lanes share a ray (G = 1
//      from 33 rays on), lane l works on ray l / G and on the chunk's edges l % G, l % G + G, ...; more than 64 / G rays
//      take several passes.  Lanes of one ray read different edges, lanes of different rays the same ones (a broadcast).
//      With several passes and several chunks the chunks are staged again for every pass: staging is one global read per
//      edge, a pass is 64 / G tests per edge;
//   5. finishes a ray with an in-wave lexicographic min over (t, row) by xor shuffles across its G lanes -- no atomics --
//      and leaves the reading's output bits in LDS;
//   6. stores the [rays, 2] block with consecutive lanes writing consecutive dwords (float16: one dword per ray).
// No cull: a per-sprite bound against the ray would have to be proven never to change a result (inclusive ends, NaN
// vertices, t <= max_range at the rounding of one division); it is left out rather than argued.
//
// The host model needs the cross-lane steps too, so the wave function is written once over the lane model of
// moog_wave_model.h.
#ifndef MOOG_RAY_SENSOR_H_
#define MOOG_RAY_SENSOR_H_

#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "moog_sprite_table.h"
#include "moog_wave_model.h"

#define MOOG_RS_CHUNK 128                                     // edges staged at a time
#define MOOG_RS_ROWS_PER_LANE (MOOG_MAX_SLOTS / MOOG_WAVE_LANES)
#define MOOG_RS_NO_KEY 0x7fffffff

// ---- descriptors -------------------------------------------------------------------------------------------------------
// One sensor of a launch.  `rows` (device memory for the kernel): per row slot | id << 16, the slot's first vertex
// (program.slot_voff) and its vertex capacity (slot_vcap).  `dirs`: [n_rays][2].
struct RsSensor {
  void* out;   // [n_envs][n_rays][2] of dtype
  const int32_t* rows;
  const double* dirs;
  double max_range;
  int32_t n_rows, n_rays, origin_slot, flags, dtype;
};
// The kernel's arguments, by value.
struct RsArgs {
  const double* f64;
  const int32_t* i32;
  int64_t f64_per_env, i32_per_env;
  int32_t n_envs, n_sensors, chunk;   // chunk: 1 .. MOOG_RS_CHUNK (the kernel's launches use MOOG_RS_CHUNK)
  int32_t o_flags, o_nverts, o_opacity, o_pos, o_angle, o_verts;
  RsSensor s[MOOG_MAX_SENSORS];
};
struct alignas(16) RsEdge {
  double wx, wy, ex, ey;
};
// A workgroup's LDS.
struct alignas(16) RsLds {
  RsEdge edge[MOOG_RS_CHUNK];
  int32_t key[MOOG_RS_CHUNK];           // row | id << 16
  int32_t estart[MOOG_MAX_SLOTS + 1];   // the first edge of every row; [MOOG_MAX_SLOTS]: the env's edge count
  uint32_t res[2 * MOOG_MAX_RAYS];      // per ray the output bits of the distance and of the id
  double cs[2];
};

// Fills `d` (everything but out / rows / dirs) and `rows` [3 * n_rows] from a sensor description; returns NULL, or why the
// description is refused.
static inline const char* moog_rs_describe(const moog_program_t* P, const moog_layout_t* L, const moog_sensor_t* T, RsSensor* d,
                                           int32_t* rows) {
  if (T->n_rays < 1 || T->n_rays > MOOG_MAX_RAYS) return "ray sensor: n_rays outside 1 .. MOOG_MAX_RAYS";
  if (T->n_rows < 1 || T->n_rows > MOOG_MAX_SLOTS) return "ray sensor: n_rows outside 1 .. MOOG_MAX_SLOTS";
  if (T->mode != MOOG_SENSOR_INSTANCE && T->mode != MOOG_SENSOR_LAYER) return "ray sensor: mode is neither MOOG_SENSOR_INSTANCE nor MOOG_SENSOR_LAYER";
  if (T->dtype != MOOG_TABLE_F32 && T->dtype != MOOG_TABLE_F16) return "ray sensor: dtype is neither MOOG_TABLE_F32 nor MOOG_TABLE_F16";
  if (T->mode == MOOG_SENSOR_INSTANCE && T->n_rows > 255) return "ray sensor: more than 255 rows in instance mode (an id is 1 .. 255)";
  if (T->flags & ~(MOOG_SENSOR_FOLLOW_ANGLE | MOOG_SENSOR_VISIBLE_ONLY)) return "ray sensor: unknown flag bits";
  if (!(T->max_range > 0.0 && T->max_range <= DBL_MAX)) return "ray sensor: max_range is not a finite number above 0";
  if (T->dtype == MOOG_TABLE_F16 && T->max_range > 65504.0) return "ray sensor: max_range above 65504 reads inf as float16";
  if (T->origin_slot < 0 || T->origin_slot >= L->S) return "ray sensor: the origin slot is outside the layout (0 .. n_slots - 1)";
  for (int k = 0; k < T->n_rays; ++k)
    for (int c = 0; c < 2; ++c)
      if (!(fabs(T->dirs[k][c]) <= DBL_MAX)) return "ray sensor: a direction is not finite";
  uint8_t seen[MOOG_MAX_SLOTS];
  memset(seen, 0, sizeof seen);
  int32_t id = 0;
  for (int r = 0; r < T->n_rows; ++r) {
    const int32_t s = T->row_slot[r];
    if (s < 0 || s >= L->S) return "ray sensor: a row's slot is outside the layout (0 .. n_slots - 1)";
    if (seen[s]) return "ray sensor: a slot is named by two rows";
    seen[s] = 1;
    if (T->mode == MOOG_SENSOR_INSTANCE) id = r + 1;
    else if (r == 0 || P->slot_layer[s] != P->slot_layer[T->row_slot[r - 1]]) ++id;   // (rows come layer after layer)
    rows[3 * r] = s | (id << 16);
    rows[3 * r + 1] = P->slot_voff[s];
    rows[3 * r + 2] = P->slot_vcap[s];
  }
  d->max_range = T->max_range;
  d->n_rows = T->n_rows; d->n_rays = T->n_rays; d->origin_slot = T->origin_slot; d->flags = T->flags; d->dtype = T->dtype;
  return nullptr;
}

// Everything of `a` but the sensors, from a layout.
static inline void moog_rs_args(const moog_layout_t* L, const double* f64, const int32_t* i32, int32_t n_envs, RsArgs* a) {
  memset(a, 0, sizeof *a);
  a->f64 = f64; a->i32 = i32; a->f64_per_env = L->f64_per_env; a->i32_per_env = L->i32_per_env;
  a->n_envs = n_envs; a->chunk = MOOG_RS_CHUNK;
  a->o_flags = L->o_flags; a->o_nverts = L->o_nverts; a->o_opacity = L->o_opacity;
  a->o_pos = L->o_pos; a->o_angle = L->o_angle; a->o_verts = L->o_verts;
}

// ---- the per-lane pieces -----------------------------------------------------------------------------------------------
// Edges of row r in the env whose int32 words are q: its vertex count when the row's slot is a target, else 0.  (A vertex
// count beyond the slot's capacity, which no kernel writes, is cut to the capacity: the reads stay inside the record.)
MOOG_ST_HD int32_t moog_rs_row_edges(const RsArgs& a, const RsSensor& s, const int32_t* q, int32_t r) {
  const int32_t slot = s.rows[3 * r] & 0xffff;
  if (slot == s.origin_slot || !(q[a.o_flags + slot] & MOOG_F_ALIVE)) return 0;
  if ((s.flags & MOOG_SENSOR_VISIBLE_ONLY) && !(q[a.o_opacity + slot] > 0)) return 0;
  int32_t n = q[a.o_nverts + slot];
  const int32_t cap = s.rows[3 * r + 2];
  if (n > cap) n = cap;
  return n >= 2 ? n : 0;
}

// Edge e of the env (numbered by lds.estart) into place j of the chunk.
MOOG_ST_HD void moog_rs_stage(const RsArgs& a, const RsSensor& s, const double* f, RsLds& lds, int32_t e, int32_t j, double ox,
                              double oy) {
  int32_t lo = 0, hi = s.n_rows;   // the last row with estart[row] <= e: rows without edges before it share its start
  while (hi - lo > 1) {
    const int32_t mid = (lo + hi) >> 1;
    if (lds.estart[mid] <= e) lo = mid; else hi = mid;
  }
  const int32_t v = e - lds.estart[lo];
  const int32_t n = lds.estart[lo + 1] - lds.estart[lo];
  const int32_t w = v + 1 == n ? 0 : v + 1;
  const double* V = f + a.o_verts + 2 * (int64_t)s.rows[3 * lo + 1];
  const double ax = V[2 * v], ay = V[2 * v + 1], bx = V[2 * w], by = V[2 * w + 1];
  RsEdge g;
  g.wx = ax - ox; g.wy = ay - oy; g.ex = bx - ax; g.ey = by - ay;
  lds.edge[j] = g;
  lds.key[j] = lo | (s.rows[3 * lo] & ~0xffff);
}

// (t, key) before (bt, bk): the smaller distance, then the lower row.
MOOG_ST_HD bool moog_rs_before(double t, int32_t key, double bt, int32_t bk) {
  return t < bt || (t == bt && (key & 0xffff) < (bk & 0xffff));
}

// Ray (dx, dy) against one staged edge; a kept hit that comes before (bt, bk) replaces it.
MOOG_ST_HD void moog_rs_test(const RsEdge& g, int32_t key, double dx, double dy, double max_range, double& bt, int32_t& bk) {
  const double den = dx * g.ey - dy * g.ex;
  const double nt = g.wx * g.ey - g.wy * g.ex;
  const double nu = g.wx * dy - g.wy * dx;
  const double ad = fabs(den);
  if (!(ad > 0.0 && ad <= DBL_MAX)) return;
  const bool pos = den > 0.0;
  const double snt = pos ? nt : -nt, snu = pos ? nu : -nu;   // sg * nt, sg * nu; sg * den is ad
  if (!(snt >= 0.0)) return;
  if (!(snu >= 0.0 && snu <= ad)) return;
  const double t = nt / den;
  if (!(t <= max_range)) return;
  if (moog_rs_before(t, key, bt, bk)) { bt = t; bk = key; }
}

MOOG_ST_HD uint32_t moog_rs_cast(double v, int32_t dtype) {
  const uint64_t b = moog_st_bits_of(v);
  return dtype == MOOG_TABLE_F16 ? moog_st_f64_to_f16_bits(b) : moog_st_f64_to_f32_bits(b);
}

// ---- the wave function -------------------------------------------------------------------------------------------------
// cos / sin of the origin's angle: the device's.  (The host model defines this before it includes the header, to rotate by
// the values a test hands it instead of this machine's libm.)
#ifndef MOOG_RS_COSSIN
#define MOOG_RS_COSSIN(ang, c, s) ((c) = cos(ang), (s) = sin(ang))
#endif

// Sensor s of env `env`, by one wave: tid is the thread's lane on the device and unused on the host, where one call runs
// all 64 lanes.
MOOG_ST_HD void moog_rs_wave(const RsArgs& a, const RsSensor& s, int64_t env, RsLds& lds, int tid) {
  const int32_t* q = a.i32 + env * a.i32_per_env;
  const double* f = a.f64 + env * a.f64_per_env;
  const bool alive = (q[a.o_flags + s.origin_slot] & MOOG_F_ALIVE) != 0;
  const double ox = f[a.o_pos + 2 * s.origin_slot], oy = f[a.o_pos + 2 * s.origin_slot + 1];
  const bool follow = (s.flags & MOOG_SENSOR_FOLLOW_ANGLE) != 0;
  if (follow) {
    MOOG_WAVE_EACH_LANE {
      if (lane == 0) {
        const double ang = f[a.o_angle + s.origin_slot];
        MOOG_RS_COSSIN(ang, lds.cs[0], lds.cs[1]);
      }
    }
  }
  // the rows' edge counts, prefix-summed: four rows a lane, then a scan of the lanes' sums
  int32_t tot[MOOG_WAVE_NP], inc[MOOG_WAVE_NP], up[MOOG_WAVE_NP];
  MOOG_WAVE_EACH_LANE {
    int32_t sum = 0;
    for (int j = 0; j < MOOG_RS_ROWS_PER_LANE; ++j) {
      const int32_t r = MOOG_RS_ROWS_PER_LANE * lane + j;
      lds.estart[r] = sum;
      if (alive && r < s.n_rows) sum += moog_rs_row_edges(a, s, q, r);
    }
    tot[MOOG_WAVE_P] = inc[MOOG_WAVE_P] = sum;
  }
  for (int d = 1; d < MOOG_WAVE_LANES; d <<= 1) {
    MOOG_WAVE_EACH_LANE up[MOOG_WAVE_P] = MOOG_WAVE_SHFL_UP(inc, d);
    MOOG_WAVE_EACH_LANE if (lane >= d) inc[MOOG_WAVE_P] += up[MOOG_WAVE_P];
  }
  MOOG_WAVE_EACH_LANE {
    const int32_t base = inc[MOOG_WAVE_P] - tot[MOOG_WAVE_P];
    for (int j = 0; j < MOOG_RS_ROWS_PER_LANE; ++j) lds.estart[MOOG_RS_ROWS_PER_LANE * lane + j] += base;
    if (lane == MOOG_WAVE_LANES - 1) lds.estart[MOOG_MAX_SLOTS] = inc[MOOG_WAVE_P];
  }
  MOOG_WAVE_SYNC();
  const int32_t N = lds.estart[MOOG_MAX_SLOTS];
  const double c = follow ? lds.cs[0] : 1.0, sn = follow ? lds.cs[1] : 0.0;

  const int32_t R = s.n_rays;
  int32_t G = 1;
  while (2 * G * R <= MOOG_WAVE_LANES) G *= 2;
  const int32_t per_pass = MOOG_WAVE_LANES / G;
  for (int32_t ray0 = 0; ray0 < R; ray0 += per_pass) {
    double dx[MOOG_WAVE_NP], dy[MOOG_WAVE_NP], bt[MOOG_WAVE_NP], ot[MOOG_WAVE_NP];
    int32_t bk[MOOG_WAVE_NP], ok[MOOG_WAVE_NP];
    MOOG_WAVE_EACH_LANE {
      const int32_t ray = ray0 + lane / G;
      double x = 0.0, y = 0.0;
      if (ray < R) { x = s.dirs[2 * ray]; y = s.dirs[2 * ray + 1]; }
      if (follow) {
        const double rx = c * x - sn * y, ry = sn * x + c * y;
        x = rx; y = ry;
      }
      dx[MOOG_WAVE_P] = x; dy[MOOG_WAVE_P] = y;
      bt[MOOG_WAVE_P] = (double)INFINITY; bk[MOOG_WAVE_P] = MOOG_RS_NO_KEY;
    }
    for (int32_t e0 = 0; e0 < N; e0 += a.chunk) {
      const int32_t nc = N - e0 < a.chunk ? N - e0 : a.chunk;
      if (ray0 == 0 || N > a.chunk) {   // (an env of one chunk stays staged for every pass)
        MOOG_WAVE_SYNC();
        MOOG_WAVE_EACH_LANE
          for (int32_t j = lane; j < nc; j += MOOG_WAVE_LANES) moog_rs_stage(a, s, f, lds, e0 + j, j, ox, oy);
        MOOG_WAVE_SYNC();
      }
      MOOG_WAVE_EACH_LANE {
        if (ray0 + lane / G < R)
          for (int32_t j = lane & (G - 1); j < nc; j += G)
            moog_rs_test(lds.edge[j], lds.key[j], dx[MOOG_WAVE_P], dy[MOOG_WAVE_P], s.max_range, bt[MOOG_WAVE_P], bk[MOOG_WAVE_P]);
      }
    }
    for (int32_t m = G >> 1; m; m >>= 1) {   // the lexicographic min over a ray's G lanes
      MOOG_WAVE_EACH_LANE { ot[MOOG_WAVE_P] = MOOG_WAVE_SHFL_XOR(bt, m); ok[MOOG_WAVE_P] = MOOG_WAVE_SHFL_XOR(bk, m); }
      MOOG_WAVE_EACH_LANE
        if (moog_rs_before(ot[MOOG_WAVE_P], ok[MOOG_WAVE_P], bt[MOOG_WAVE_P], bk[MOOG_WAVE_P])) { bt[MOOG_WAVE_P] = ot[MOOG_WAVE_P]; bk[MOOG_WAVE_P] = ok[MOOG_WAVE_P]; }
    }
    MOOG_WAVE_EACH_LANE {
      const int32_t ray = ray0 + lane / G;
      if ((lane & (G - 1)) == 0 && ray < R) {
        const bool hit = bk[MOOG_WAVE_P] != MOOG_RS_NO_KEY;
        lds.res[2 * ray] = moog_rs_cast(hit ? bt[MOOG_WAVE_P] + 0.0 : s.max_range, s.dtype);
        lds.res[2 * ray + 1] = moog_rs_cast(hit ? (double)(bk[MOOG_WAVE_P] >> 16) : 0.0, s.dtype);
      }
    }
  }
  MOOG_WAVE_SYNC();
  MOOG_WAVE_EACH_LANE {
    if (s.dtype == MOOG_TABLE_F32) {
      uint32_t* out = (uint32_t*)s.out + env * (2 * R);
      for (int32_t j = lane; j < 2 * R; j += MOOG_WAVE_LANES) out[j] = lds.res[j];
    } else {
      uint32_t* out = (uint32_t*)s.out + env * R;
      for (int32_t j = lane; j < R; j += MOOG_WAVE_LANES) out[j] = lds.res[2 * j] | (lds.res[2 * j + 1] << 16);
    }
  }
}

#if defined(__HIPCC__)
void moog_ray_sensor_launch(RsArgs a, hipStream_t stream);   // moog_ray_sensor.hip
#endif

#endif  // MOOG_RAY_SENSOR_H_
