// moog_wave_model.h -- the lane model of the observers' wave functions (moog_ray_sensor.h moog_rs_wave, moog_contacts.h
// moog_ct_wave / moog_ct_narrow): one text that a wavefront runs on the device and that a host model walks lane by lane.
//
// The host models (tests/csrc) need the cross-lane steps too, so a wave function is written once over these macros.  It
// takes `int tid`, the thread's lane on the device and unused on the host, where one call runs all 64 lanes:
//   MOOG_WAVE_EACH_LANE  a "for every lane" block, with `lane` in scope: on the device it runs for the lane the thread is, on
//                        the host it loops over MOOG_WAVE_LANES lanes;
//   MOOG_WAVE_NP / _P    per-lane variables are `T v[MOOG_WAVE_NP]`, indexed `v[MOOG_WAVE_P]` inside a block: scalars on the
//                        device (one element, index 0), arrays of one element per lane on the host;
//   MOOG_WAVE_SYNC()     the workgroup barrier (a workgroup is one wavefront); nothing on the host, whose blocks run in order;
//   MOOG_WAVE_SHFL_XOR / _SHFL_UP / _BALLOT   take the per-lane variable: a shuffle or a ballot on the device, on the host a
//                        read of the other lane's element or a loop over the lanes (int32_t flags);
//   MOOG_WAVE_POPC       the population count of a ballot.
// Why the host loop sees what the wavefront sees: every shuffle sits in a block of its own that only reads the variable it
// shuffles and writes another, and a ballot stands between blocks, so the host reads the values from before the step, as the
// lanes of a wave do.
#ifndef MOOG_WAVE_MODEL_H_
#define MOOG_WAVE_MODEL_H_

#include <stdint.h>

#define MOOG_WAVE_LANES 64

#if defined(__HIP_DEVICE_COMPILE__)
#define MOOG_WAVE_NP 1
#define MOOG_WAVE_EACH_LANE for (int lane = tid, once_ = 1; once_; once_ = 0)
#define MOOG_WAVE_P 0
#define MOOG_WAVE_SYNC() __syncthreads()
#define MOOG_WAVE_SHFL_XOR(arr, m) __shfl_xor((arr)[0], (m))
#define MOOG_WAVE_SHFL_UP(arr, d) __shfl_up((arr)[0], (d))
#define MOOG_WAVE_BALLOT(arr) ((uint64_t)__ballot((arr)[0] != 0))
#define MOOG_WAVE_POPC(m) __popcll(m)
#else
#define MOOG_WAVE_NP MOOG_WAVE_LANES
#define MOOG_WAVE_EACH_LANE for (int lane = 0; lane < MOOG_WAVE_LANES; ++lane)
#define MOOG_WAVE_P lane
#define MOOG_WAVE_SYNC() (void)tid
#define MOOG_WAVE_SHFL_XOR(arr, m) (arr)[lane ^ (m)]
#define MOOG_WAVE_SHFL_UP(arr, d) (arr)[lane >= (d) ? lane - (d) : lane]
static inline uint64_t moog_wave_host_ballot(const int32_t* v) {
  uint64_t m = 0;
  for (int k = 0; k < MOOG_WAVE_LANES; ++k) if (v[k]) m |= 1ull << k;
  return m;
}
#define MOOG_WAVE_BALLOT(arr) moog_wave_host_ballot(arr)
#define MOOG_WAVE_POPC(m) __builtin_popcountll(m)
#endif

#endif  // MOOG_WAVE_MODEL_H_
