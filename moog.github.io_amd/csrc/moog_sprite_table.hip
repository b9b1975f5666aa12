// moog_sprite_table.hip -- the sprite-table kernel (moog_sprite_table.h has the design and the code it runs), its own
// translation unit: nothing of the step, reset or raster kernels is compiled here.
#include <hip/hip_runtime.h>

#include "moog_sprite_table.h"

// Grid: x = the tables' workgroups one after the other (StTable::blk0), y = the chunk of envs.  A workgroup belongs to one
// table, so the table's descriptor is wave-uniform; only the column descriptor is read per lane.
__global__ __launch_bounds__(MOOG_ST_THREADS) void moog_sprite_table_kernel(StArgs a) {
  int ti = 0;
  for (int k = 1; k < a.n_tables; ++k)
    if (blockIdx.x >= a.t[k].blk0) ti = k;
  const StTable& t = a.t[ti];
  moog_st_lane(a, t, blockIdx.y, (blockIdx.x - t.blk0) * MOOG_ST_THREADS + threadIdx.x);
}

// One launch for every table of `a` (n_tables >= 1, every t[k].out bound); fills chunk_envs and the tables' blk0.
void moog_sprite_table_launch(StArgs a, hipStream_t stream) {
  a.chunk_envs = moog_st_chunk_envs(&a);
  uint32_t blocks = 0;
  for (int k = 0; k < a.n_tables; ++k) {
    a.t[k].blk0 = blocks;
    blocks += moog_st_blocks(&a.t[k], a.chunk_envs);
  }
  const uint32_t chunks = (uint32_t)((a.n_envs + a.chunk_envs - 1) / a.chunk_envs);
  hipLaunchKernelGGL(moog_sprite_table_kernel, dim3(blocks, chunks), dim3(MOOG_ST_THREADS), 0, stream, a);
}
