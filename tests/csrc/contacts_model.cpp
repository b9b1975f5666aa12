// Host model of the contacts kernel: csrc/moog_contacts.h -- the descriptors and the wave function the kernel runs -- compiled
// with g++ -O2 -ffp-contract=off, the launch's grid walked wave by wave, every wave lane by lane, over host records
// (tests/test_contacts_host.py).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../moog.github.io_amd/csrc/moog_contacts.h"

extern "C" {

// Every observer of obs[0 .. n_obs) over n_envs host records, as ONE launch of the kernel does it: grid x = env,
// y = observer, moog_ct_wave per workgroup.  out[k]: observer k's buffer (any byte alignment).  chunk > 0 overrides the
// candidates held at a time (1 .. MOOG_CT_CHUNK).  n_cand != NULL: [n_obs][n_envs] candidates past the broad phase.
// Returns 0, or -1 with the reason in err.
int ct_model_observe(const moog_program_t* P, const moog_contacts_t* obs, int n_obs, const double* f64, const int32_t* i32,
                     int n_envs, void* const* out, int chunk, int32_t* n_cand, char* err, int err_len) {
  moog_layout_t L;
  moog_layout(P, &L);
  static int32_t rows[MOOG_MAX_CONTACTS][3 * 2 * MOOG_MAX_SLOTS];
  CtArgs a;
  moog_ct_args(&L, f64, i32, n_envs, &a);
  if (n_obs < 1 || n_obs > MOOG_MAX_CONTACTS) { snprintf(err, err_len, "at most MOOG_MAX_CONTACTS contacts observers per engine"); return -1; }
  size_t lds_bytes = 0;
  for (int k = 0; k < n_obs; ++k) {
    const char* why = moog_ct_describe(P, &L, &obs[k], &a.c[k], rows[k]);
    if (why) { snprintf(err, err_len, "%s", why); return -1; }
    a.c[k].rows = rows[k];
    a.c[k].out = (uint8_t*)out[k];
    if (moog_ct_lds_bytes(a.c[k]) > lds_bytes) lds_bytes = moog_ct_lds_bytes(a.c[k]);
  }
  a.n_obs = n_obs;
  if (chunk > 0) {
    if (chunk > MOOG_CT_CHUNK) { snprintf(err, err_len, "chunk above MOOG_CT_CHUNK"); return -1; }
    a.chunk = chunk;
  }
  if (lds_bytes > 65536) { snprintf(err, err_len, "more than 64 KB of LDS"); return -1; }
  void* lds = aligned_alloc(16, (lds_bytes + 15) & ~(size_t)15);
  for (int y = 0; y < n_obs; ++y)
    for (int64_t env = 0; env < n_envs; ++env) {
      memset(lds, 0xff, lds_bytes);   // (LDS holds anything when a workgroup starts)
      const int32_t seen = moog_ct_wave(a, a.c[y], env, lds, 0);
      if (n_cand) n_cand[(int64_t)y * n_envs + env] = seen;
    }
  free(lds);
  return 0;
}

// (n0, n1, n_layers1, same) of a description, or -1 with the reason in err.
int ct_model_shape(const moog_program_t* P, const moog_contacts_t* obs, int32_t* shape, char* err, int err_len) {
  moog_layout_t L;
  moog_layout(P, &L);
  static int32_t rows[3 * 2 * MOOG_MAX_SLOTS];
  CtObs d;
  memset(&d, 0, sizeof d);
  const char* why = moog_ct_describe(P, &L, obs, &d, rows);
  if (why) { snprintf(err, err_len, "%s", why); return -1; }
  shape[0] = d.n0; shape[1] = d.n1; shape[2] = d.n_layers1; shape[3] = d.same;
  return 0;
}

int ct_model_chunk(void) { return MOOG_CT_CHUNK; }

}  // extern "C"
