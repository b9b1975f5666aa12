// moog_ray_sensor.hip -- the ray-sensor kernel (moog_ray_sensor.h has the design and the code it runs), its own translation
// unit: nothing of the step, reset or raster kernels is compiled here.
#include <hip/hip_runtime.h>

#include "moog_ray_sensor.h"

// Grid: x = env, y = sensor; a workgroup is one wavefront.
__global__ __launch_bounds__(MOOG_WAVE_LANES) void moog_ray_sensor_kernel(RsArgs a) {
  __shared__ RsLds lds;
  moog_rs_wave(a, a.s[blockIdx.y], (int64_t)blockIdx.x, lds, (int)threadIdx.x);
}

// One launch for every sensor of `a` (n_sensors >= 1, every s[k].out bound).
void moog_ray_sensor_launch(RsArgs a, hipStream_t stream) {
  a.chunk = MOOG_RS_CHUNK;
  hipLaunchKernelGGL(moog_ray_sensor_kernel, dim3((uint32_t)a.n_envs, (uint32_t)a.n_sensors), dim3(MOOG_WAVE_LANES), 0, stream, a);
}
