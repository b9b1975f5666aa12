// moog_contacts.hip -- the contacts kernel (moog_contacts.h has the design and the code it runs), its own translation unit:
// nothing of the step, reset or raster kernels is compiled here.
#include <hip/hip_runtime.h>

#include "moog_contacts.h"

// Grid: x = env, y = observer; a workgroup is one wavefront.  The dynamic LDS block is sized for the launch's largest observer.
__global__ __launch_bounds__(MOOG_WAVE_LANES) void moog_contacts_kernel(CtArgs a) {
  extern __shared__ double moog_ct_lds[];
  moog_ct_wave(a, a.c[blockIdx.y], (int64_t)blockIdx.x, moog_ct_lds, (int)threadIdx.x);
}

// One launch for every observer of `a` (n_obs >= 1, every c[k].out bound).
void moog_contacts_launch(CtArgs a, hipStream_t stream) {
  a.chunk = MOOG_CT_CHUNK;
  size_t lds = 0;
  for (int k = 0; k < a.n_obs; ++k) {
    const size_t b = moog_ct_lds_bytes(a.c[k]);
    if (b > lds) lds = b;
  }
  hipLaunchKernelGGL(moog_contacts_kernel, dim3((uint32_t)a.n_envs, (uint32_t)a.n_obs), dim3(MOOG_WAVE_LANES), lds, stream, a);
}
