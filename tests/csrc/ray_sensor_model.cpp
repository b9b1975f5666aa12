// Host model of the ray-sensor kernel: csrc/moog_ray_sensor.h -- the descriptors and the wave function the kernel runs --
// compiled with g++ -O2 -ffp-contract=off, the launch's grid walked wave by wave, every wave lane by lane, over host records
// (tests/test_ray_sensor_host.py).
#include <stdint.h>
#include <stdio.h>

// cos / sin of the origin's angle: what the caller hands over for the env under way (g_cs), else libm's
static const double* g_cs = nullptr;
static void rs_model_cossin(double ang, double& c, double& s);
#define MOOG_RS_COSSIN(ang, c, s) rs_model_cossin((ang), (c), (s))

#include "../../moog.github.io_amd/csrc/moog_ray_sensor.h"

static void rs_model_cossin(double ang, double& c, double& s) {
  if (g_cs) { c = g_cs[0]; s = g_cs[1]; }
  else { c = cos(ang); s = sin(ang); }
}

extern "C" {

// Every sensor of sensors[0 .. n_sensors) over n_envs host records, as ONE launch of the kernel does it: grid x = env,
// y = sensor, moog_rs_wave per workgroup.  out[k]: sensor k's buffer.  chunk > 0 overrides the edges staged at a time
// (1 .. MOOG_RS_CHUNK).  cs != NULL: [n_sensors][n_envs][2] cos / sin of the origin's angle to rotate by instead of this
// machine's libm.  Returns 0, or -1 with the reason in err.
int rs_model_cast(const moog_program_t* P, const moog_sensor_t* sensors, int n_sensors, const double* f64, const int32_t* i32,
                  int n_envs, void* const* out, int chunk, const double* cs, char* err, int err_len) {
  moog_layout_t L;
  moog_layout(P, &L);
  static int32_t rows[MOOG_MAX_SENSORS][3 * MOOG_MAX_SLOTS];
  RsArgs a;
  moog_rs_args(&L, f64, i32, n_envs, &a);
  if (n_sensors < 1 || n_sensors > MOOG_MAX_SENSORS) { snprintf(err, err_len, "at most MOOG_MAX_SENSORS ray sensors per engine"); return -1; }
  for (int k = 0; k < n_sensors; ++k) {
    const char* why = moog_rs_describe(P, &L, &sensors[k], &a.s[k], rows[k]);
    if (why) { snprintf(err, err_len, "%s", why); return -1; }
    a.s[k].rows = rows[k];
    a.s[k].dirs = &sensors[k].dirs[0][0];
    a.s[k].out = out[k];
  }
  a.n_sensors = n_sensors;
  if (chunk > 0) {
    if (chunk > MOOG_RS_CHUNK) { snprintf(err, err_len, "chunk above MOOG_RS_CHUNK"); return -1; }
    a.chunk = chunk;
  }
  static RsLds lds;
  for (int y = 0; y < n_sensors; ++y)
    for (int64_t env = 0; env < n_envs; ++env) {
      memset(&lds, 0xff, sizeof lds);   // (LDS holds anything when a workgroup starts)
      g_cs = cs ? cs + 2 * ((int64_t)y * n_envs + env) : nullptr;
      moog_rs_wave(a, a.s[y], env, lds, 0);
    }
  g_cs = nullptr;
  return 0;
}

int rs_model_chunk(void) { return MOOG_RS_CHUNK; }

}  // extern "C"
