// Host model of the sprite-table kernel: csrc/moog_sprite_table.h -- the conversions, the descriptors and the lane function
// the kernel runs -- compiled with g++, the launch's grid walked lane by lane over host records
// (tests/test_sprite_table_host.py).
#include <stdint.h>
#include <stdio.h>

#include "../../moog.github.io_amd/csrc/moog_sprite_table.h"

extern "C" {

// float64 bit patterns -> float32 and float16 bit patterns, with the header's conversions
void st_model_convert(const uint64_t* in, int64_t n, uint32_t* f32, uint16_t* f16) {
  for (int64_t i = 0; i < n; ++i) {
    f32[i] = moog_st_f64_to_f32_bits(in[i]);
    f16[i] = (uint16_t)moog_st_f64_to_f16_bits(in[i]);
  }
}

// Every table of tables[0 .. n_tables) over n_envs host records, as ONE launch of the kernel does it: the same grid
// (moog_st_chunk_envs / moog_st_blocks; chunk_envs > 0 overrides the chunk size, to walk the several-chunk path with few
// envs), every lane of every workgroup through moog_st_lane.  out[k]: table k's buffer.  Returns 0, or -1 with the reason
// in err.
int st_model_pack(const moog_program_t* P, const moog_table_t* tables, int n_tables, const double* f64, const int32_t* i32,
                  int n_envs, void* const* out, int chunk_envs, char* err, int err_len) {
  moog_layout_t L;
  moog_layout(P, &L);
  static int32_t rows[MOOG_MAX_TABLES][MOOG_MAX_SLOTS];
  StArgs a;
  memset(&a, 0, sizeof a);
  if (n_tables < 1 || n_tables > MOOG_MAX_TABLES) { snprintf(err, err_len, "at most MOOG_MAX_TABLES sprite tables"); return -1; }
  for (int k = 0; k < n_tables; ++k) {
    const char* why = moog_st_describe(P, &L, &tables[k], &a.t[k], rows[k]);
    if (why) { snprintf(err, err_len, "%s", why); return -1; }
    a.t[k].rows = rows[k];
    a.t[k].out = out[k];
  }
  a.f64 = f64; a.i32 = i32; a.f64_per_env = L.f64_per_env; a.i32_per_env = L.i32_per_env;
  a.n_envs = n_envs; a.o_flags = L.o_flags; a.n_tables = n_tables;
  a.chunk_envs = chunk_envs > 0 ? chunk_envs : moog_st_chunk_envs(&a);
  uint32_t blocks = 0;
  for (int k = 0; k < n_tables; ++k) { a.t[k].blk0 = blocks; blocks += moog_st_blocks(&a.t[k], a.chunk_envs); }
  const uint32_t chunks = (uint32_t)((n_envs + a.chunk_envs - 1) / a.chunk_envs);
  for (uint32_t y = 0; y < chunks; ++y)
    for (uint32_t bx = 0; bx < blocks; ++bx) {
      int ti = 0;
      for (int k = 1; k < a.n_tables; ++k) if (bx >= a.t[k].blk0) ti = k;
      for (uint32_t tid = 0; tid < MOOG_ST_THREADS; ++tid)
        moog_st_lane(a, a.t[ti], y, (bx - a.t[ti].blk0) * MOOG_ST_THREADS + tid);
    }
  return 0;
}

}  // extern "C"
