// moog_sprite_table.h -- sprite tables (the SpriteTable observer; include/moog_engine.h moog_engine_add_table): the element
// function the kernel of moog_sprite_table.hip runs per output element, the two conversions it needs, and the host code that
// turns a moog_table_t into the kernel's descriptors.  Everything here is host AND device code: tests/csrc/sprite_table_model.cpp
// compiles this header with g++ and runs the same functions over host records (tests/test_sprite_table_host.py).
//
// The mapping is output-major: one output element (float32) or one aligned pair of elements (float16) per lane, so that a
// wave's stores are 64 consecutive dwords.  From its element index a lane derives (env, row, column); the column descriptor
// says which array of the env's record the value comes from, the row descriptor which slot.  Gathers stay inside one record.
#ifndef MOOG_SPRITE_TABLE_H_
#define MOOG_SPRITE_TABLE_H_

#include <stdint.h>
#include <string.h>

#include "../../include/moog_engine.h"

#if defined(__HIPCC__)
#define MOOG_ST_HD __host__ __device__ static inline
#else
#define MOOG_ST_HD static inline
#endif

// ---- conversions -------------------------------------------------------------------------------------------------------
// float64 bits -> the bits of the nearest value of a binary format with EB exponent and MB mantissa bits, ties to even, in ONE
// rounding, on the integers: what numpy.ndarray.astype gives.  (float64 -> float32 -> float16 rounds twice and misses the
// float16 ties' neighbours: 1 + 2^-11 + 2^-30 becomes 1.0 instead of 1 + 2^-10.  Integer code also does not depend on the
// denormal mode a kernel runs under.)  Overflow gives inf, inf passes through, NaN stays NaN (quiet, leading payload bits
// kept), values below half the smallest subnormal give a signed zero.
template <int EB, int MB>
MOOG_ST_HD uint32_t moog_st_round_bits(uint64_t b) {
  const uint32_t sign = (uint32_t)(b >> 63) << (EB + MB);
  const int32_t e = (int32_t)((b >> 52) & 0x7ff);
  const uint64_t m = b & 0xfffffffffffffull;
  const uint32_t emax = (1u << EB) - 1u;
  if (e == 0x7ff) {
    if (m) return sign | (emax << MB) | (1u << (MB - 1)) | (uint32_t)(m >> (52 - MB));
    return sign | (emax << MB);
  }
  if (e == 0) return sign;   // zero, or a float64 subnormal: far below half of either format's smallest subnormal
  const int32_t t = e - 1023 + ((1 << (EB - 1)) - 1);   // the biased exponent in the target format
  if (t >= (int32_t)emax) return sign | (emax << MB);
  const uint64_t sig = m | (1ull << 52);
  int32_t shift = 52 - MB;
  uint32_t base = 0;
  if (t <= 0) {   // a subnormal of the target: the significand in units of the smallest subnormal
    shift += 1 - t;
    if (shift > 63) return sign;
  } else {
    base = (uint32_t)(t - 1) << MB;   // (the significand's leading one adds the exponent's last unit)
  }
  const uint64_t q = sig >> shift, rem = sig & ((1ull << shift) - 1ull), half = 1ull << (shift - 1);
  uint32_t r = base + (uint32_t)q;
  if (rem > half || (rem == half && (q & 1ull))) ++r;   // (a carry runs into the exponent: the next binade, or inf)
  return sign | r;
}
MOOG_ST_HD uint32_t moog_st_f64_to_f32_bits(uint64_t b) { return moog_st_round_bits<8, 23>(b); }
MOOG_ST_HD uint32_t moog_st_f64_to_f16_bits(uint64_t b) { return moog_st_round_bits<5, 10>(b); }

MOOG_ST_HD uint64_t moog_st_bits_of(double x) {
  uint64_t b;
#if defined(__HIP_DEVICE_COMPILE__)
  b = (uint64_t)__double_as_longlong(x);
#else
  memcpy(&b, &x, sizeof b);
#endif
  return b;
}

// ---- descriptors -------------------------------------------------------------------------------------------------------
// Where a column's value comes from.  F64: f64[off + stride * slot]; I32: i32[off + slot]; ALIVE: 1; LAYER: the row's layer.
enum { MOOG_ST_F64 = 0, MOOG_ST_I32 = 1, MOOG_ST_ALIVE = 2, MOOG_ST_LAYER = 3 };
struct StCol {
  int32_t off;
  int16_t stride, kind;
};
// One table of a launch.  `rows` (device memory for the kernel): slot | layer << 16 per row.
struct StTable {
  void* out;              // [n_envs][n_rows][n_cols] of dtype
  const int32_t* rows;
  uint32_t n_cols;
  uint32_t per_env;       // n_rows * n_cols
  uint32_t dtype;         // MOOG_TABLE_*
  uint32_t blk0;          // first workgroup of the table within a launch's grid row
  StCol col[MOOG_MAX_TABLE_COLS];
};
// The kernel's arguments, by value.  Envs come in chunks of `chunk_envs` (grid row y: envs y * chunk_envs ..), small enough
// that an element index within a chunk fits 32 bits whatever n_envs is.
struct StArgs {
  const double* f64;
  const int32_t* i32;
  int64_t f64_per_env, i32_per_env;
  int32_t n_envs, chunk_envs, o_flags, n_tables;
  StTable t[MOOG_MAX_TABLES];
};
#define MOOG_ST_THREADS 256
#define MOOG_ST_CHUNK_ELEMS (1u << 30)   // elements of one table in one chunk of envs, at most

// Fills `d` (everything but out / rows / blk0) and `rows` [n_rows] from a table description; returns NULL, or why the
// description is refused.
static inline const char* moog_st_describe(const moog_program_t* P, const moog_layout_t* L, const moog_table_t* T, StTable* d,
                                           int32_t* rows) {
  if (T->n_rows < 1 || T->n_rows > MOOG_MAX_SLOTS) return "sprite table: n_rows outside 1 .. MOOG_MAX_SLOTS";
  if (T->n_cols < 1 || T->n_cols > MOOG_MAX_TABLE_COLS) return "sprite table: n_cols outside 1 .. MOOG_MAX_TABLE_COLS";
  if (T->dtype != MOOG_TABLE_F32 && T->dtype != MOOG_TABLE_F16) return "sprite table: dtype is neither MOOG_TABLE_F32 nor MOOG_TABLE_F16";
  for (int r = 0; r < T->n_rows; ++r) {
    const int32_t s = T->row_slot[r];
    if (s < 0 || s >= L->S) return "sprite table: a row's slot is outside the layout (0 .. n_slots - 1)";
    rows[r] = s | (P->slot_layer[s] << 16);
  }
  for (int c = 0; c < T->n_cols; ++c) {
    StCol k = {0, 1, MOOG_ST_F64};
    switch (T->cols[c]) {
      case MOOG_TCOL_ALIVE: k.kind = MOOG_ST_ALIVE; break;
      case MOOG_TCOL_LAYER: k.kind = MOOG_ST_LAYER; break;
      case MOOG_TCOL_X: k.off = L->o_pos; k.stride = 2; break;
      case MOOG_TCOL_Y: k.off = L->o_pos + 1; k.stride = 2; break;
      case MOOG_TCOL_X_VEL: k.off = L->o_vel; k.stride = 2; break;
      case MOOG_TCOL_Y_VEL: k.off = L->o_vel + 1; k.stride = 2; break;
      case MOOG_TCOL_ANGLE: k.off = L->o_angle; break;
      case MOOG_TCOL_ANGLE_VEL: k.off = L->o_angvel; break;
      case MOOG_TCOL_MASS: k.off = L->o_mass; break;
      case MOOG_TCOL_C0: k.off = L->o_color; k.stride = 3; break;
      case MOOG_TCOL_C1: k.off = L->o_color + 1; k.stride = 3; break;
      case MOOG_TCOL_C2: k.off = L->o_color + 2; k.stride = 3; break;
      case MOOG_TCOL_SCALE:
        if (L->o_scale < 0) return "sprite table: column scale needs a program with sprite_factors (o_scale is -1)";
        k.off = L->o_scale; break;
      case MOOG_TCOL_ASPECT:
        if (L->o_aspect < 0) return "sprite table: column aspect_ratio needs a program with sprite_factors (o_aspect is -1)";
        k.off = L->o_aspect; break;
      case MOOG_TCOL_OPACITY: k.kind = MOOG_ST_I32; k.off = L->o_opacity; break;
      case MOOG_TCOL_SHAPE_ID: k.kind = MOOG_ST_I32; k.off = L->o_shape; break;
      case MOOG_TCOL_N_VERTICES: k.kind = MOOG_ST_I32; k.off = L->o_nverts; break;
      default: return "sprite table: unknown column id (MOOG_TCOL_*)";
    }
    d->col[c] = k;
  }
  d->n_cols = (uint32_t)T->n_cols;
  d->per_env = (uint32_t)(T->n_rows * T->n_cols);
  d->dtype = (uint32_t)T->dtype;
  return nullptr;
}

// Envs per chunk (see StArgs) and the workgroups one table takes per chunk: a lane per element, or per pair of float16
// elements (one more pair when the buffer starts on an odd half-word: pairs are aligned dwords of the buffer).
static inline int32_t moog_st_chunk_envs(const StArgs* a) {
  uint32_t per_env = 1;
  for (int k = 0; k < a->n_tables; ++k) if (a->t[k].per_env > per_env) per_env = a->t[k].per_env;
  const uint32_t c = MOOG_ST_CHUNK_ELEMS / per_env;
  return (int32_t)((uint32_t)a->n_envs < c ? (uint32_t)a->n_envs : c);
}
static inline uint32_t moog_st_blocks(const StTable* t, int32_t chunk_envs) {
  const uint32_t n = (uint32_t)chunk_envs * t->per_env;
  const uint32_t lanes = t->dtype == MOOG_TABLE_F16 ? n / 2u + 1u : n;
  return (lanes + MOOG_ST_THREADS - 1u) / MOOG_ST_THREADS;
}

// ---- the element function ----------------------------------------------------------------------------------------------
// Bits (float32, or float16 in the low half) of element `el` of env `env`'s rows of table t.
MOOG_ST_HD uint32_t moog_st_element(const StArgs& a, const StTable& t, int64_t env, uint32_t el) {
  const uint32_t row = el / t.n_cols, c = el - row * t.n_cols;
  const int32_t rw = t.rows[row];
  const int32_t slot = rw & 0xffff;
  const int32_t* q = a.i32 + env * a.i32_per_env;
  if (!(q[a.o_flags + slot] & MOOG_F_ALIVE)) return 0u;
  const StCol k = t.col[c];
  double v;
  if (k.kind == MOOG_ST_F64) v = a.f64[env * a.f64_per_env + k.off + (int32_t)k.stride * slot];
  else if (k.kind == MOOG_ST_I32) v = (double)q[k.off + slot];   // (exact: one rounding, below)
  else if (k.kind == MOOG_ST_ALIVE) v = 1.0;
  else v = (double)(rw >> 16);
  const uint64_t b = moog_st_bits_of(v);
  return t.dtype == MOOG_TABLE_F16 ? moog_st_f64_to_f16_bits(b) : moog_st_f64_to_f32_bits(b);
}

// What lane `lane` of table t's workgroups does in chunk `chunk` -- the whole kernel body, and the host model's inner loop.
// float32: element `lane` of the chunk.  float16: the aligned dword of the buffer that holds elements 2 * lane - head and the
// next one, head = 1 when the buffer starts in the middle of a dword; a pair's element outside the chunk is left alone (a
// 2-byte store of the other one).
MOOG_ST_HD void moog_st_lane(const StArgs& a, const StTable& t, uint32_t chunk, uint32_t lane) {
  const int64_t env0 = (int64_t)chunk * a.chunk_envs;
  const int64_t left = (int64_t)a.n_envs - env0;
  const uint32_t envs = (uint32_t)(left < (int64_t)a.chunk_envs ? left : (int64_t)a.chunk_envs);
  const uint32_t n = envs * t.per_env;   // elements of this chunk
  if (t.dtype == MOOG_TABLE_F32) {
    if (lane >= n) return;
    const uint32_t env = lane / t.per_env;
    ((uint32_t*)t.out)[env0 * t.per_env + lane] = moog_st_element(a, t, env0 + env, lane - env * t.per_env);
    return;
  }
  uint16_t* out = (uint16_t*)t.out + env0 * t.per_env;
  const uint32_t head = (uint32_t)(((uintptr_t)out >> 1) & 1u);
  const int64_t e0 = 2 * (int64_t)lane - head, e1 = e0 + 1;
  const bool in0 = e0 >= 0 && e0 < (int64_t)n, in1 = e1 < (int64_t)n;
  uint32_t lo = 0, hi = 0;
  if (in0) { const uint32_t env = (uint32_t)e0 / t.per_env; lo = moog_st_element(a, t, env0 + env, (uint32_t)e0 - env * t.per_env); }
  if (in1) { const uint32_t env = (uint32_t)e1 / t.per_env; hi = moog_st_element(a, t, env0 + env, (uint32_t)e1 - env * t.per_env); }
  if (in0 && in1) *(uint32_t*)(out + e0) = lo | (hi << 16);
  else if (in0) out[e0] = (uint16_t)lo;
  else if (in1) out[e1] = (uint16_t)hi;
}

#if defined(__HIPCC__)
void moog_sprite_table_launch(StArgs a, hipStream_t stream);   // moog_sprite_table.hip
#endif

#endif  // MOOG_SPRITE_TABLE_H_
