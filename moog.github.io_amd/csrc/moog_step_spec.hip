// moog_step_spec.hip -- the step kernel specialised for ONE program (built by moog/_spec.py, loaded by moog_engine.hip).
//   hipcc ... -DMOOG_SPEC_PROGRAM_INC='"<generated>.inc"' -DMOOG_STEP_DYN=0|1|2 -DMOOG_STEP_WPS=2|3|4 -DMOOG_SPEC_KERNEL=0|1|2 -c
//   and the three objects linked into step_<hash>_d<dyn>w<wps>.so
// The generated include defines `constexpr static const moog_program_t MOOG_SPEC_PROGRAM = {...};` and MOOG_SPEC_HASH (FNV-1a
// 64 of the program's bytes); the flattened force list is a constant derived from it (moog_fops.h), and KArgs::fops / n_fops /
// dbg are ignored.  Same source, same arithmetic as the generic kernels (moog_step_inst.hip): results are bit-identical
// (tests/test_gpu_parity.py::test_specialised_step_kernel_is_result_neutral); only what the program never uses is gone.
// Three kernels, one per unit so that they compile side by side (MOOG_SPEC_KERNEL): 0 the one-step kernel, 1 the one with the
// action-repeat loop for calls with KArgs::repeat > 1 and for action sequences (KArgs::reward_seq), 2 the one that also records
// a sequence's trajectory (KArgs::traj).  Unit 0 carries the object's interface as well.
// MOOG_SPEC_KERNEL=3 is the candidate kernel (moog_plan_step_kernel, moog_engine_plan_sequences): compiled beside the three, with
// the uncut record as its compile-time layout (MOOG_SPEC_UNCUT), and linked into an object of its own, plan_<hash>_d<dyn>w<wps>.so,
// with an interface of its own (the same checks, moog_spec_configure_3 / moog_spec_launch_3): step_<hash>_... keeps three kernels.
#include <hip/hip_runtime.h>

#define MOOG_WITH_MAZE (MOOG_STEP_DYN == 2)
#if MOOG_SPEC_KERNEL == 3
#define MOOG_SPEC_UNCUT 1
#endif
#include "moog_kernels.h"

#ifndef MOOG_SRC_DIGEST
#define MOOG_SRC_DIGEST 0ull
#endif
#define MOOG_STR2(x) #x
#define MOOG_STR(x) MOOG_STR2(x)
#if MOOG_SPEC_KERNEL == 0 || MOOG_SPEC_KERNEL == 3
extern "C" const char moog_src_digest_marker[] = "MOOG_SRC_DIGEST=" MOOG_STR(MOOG_SRC_DIGEST);   // (read as text by moog/_digest.py)

#endif

extern "C" {

#if MOOG_SPEC_KERNEL == 0 || MOOG_SPEC_KERNEL == 3

// (moog/_digest.py: the kernel sources and flags this object was built from; the engine library refuses another build's)
unsigned long long moog_spec_source_digest(void) { return MOOG_SRC_DIGEST; }
int moog_spec_abi(void) { return MOOG_ABI_VERSION; }
unsigned long long moog_spec_hash(void) { return MOOG_SPEC_HASH; }
int moog_spec_variant(void) { return MOOG_STEP_DYN | (MOOG_STEP_WPS << 8); }
unsigned long long moog_spec_kargs_size(void) { return sizeof(KArgs); }
// (the program the kernel was compiled for: the engine compares it with its own before using the kernel)
const void* moog_spec_program(void) { return &MOOG_SPEC_PROGRAM; }
#endif

#ifndef MOOG_SPEC_KERNEL
#error "MOOG_SPEC_KERNEL=0|1|2: which of the object's three kernels this unit holds; 3: the candidate kernel"
#endif
#if MOOG_SPEC_KERNEL == 3
#define MOOG_SPEC_THE_KERNEL moog_plan_step_kernel<MOOG_STEP_DYN != 0, MOOG_STEP_WPS, MOOG_STEP_DYN>
#else
#define MOOG_SPEC_THE_KERNEL moog_step_kernel<MOOG_STEP_DYN != 0, MOOG_STEP_WPS, MOOG_STEP_DYN, (MOOG_SPEC_KERNEL >= 1), (MOOG_SPEC_KERNEL >= 2)>
#endif
#define MOOG_CAT_(a, b) a##b
#define MOOG_CAT(a, b) MOOG_CAT_(a, b)

int MOOG_CAT(moog_spec_configure_, MOOG_SPEC_KERNEL)(size_t lds) {
  return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(MOOG_SPEC_THE_KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}
void MOOG_CAT(moog_spec_launch_, MOOG_SPEC_KERNEL)(int n_envs, size_t lds, hipStream_t s, const KArgs* a) {
  hipLaunchKernelGGL((MOOG_SPEC_THE_KERNEL), dim3(n_envs), dim3(MOOG_STEP_THREADS), lds, s, *a);
}

#if MOOG_SPEC_KERNEL == 0
int moog_spec_configure_1(size_t lds);
int moog_spec_configure_2(size_t lds);
void moog_spec_launch_1(int n_envs, size_t lds, hipStream_t s, const KArgs* a);
void moog_spec_launch_2(int n_envs, size_t lds, hipStream_t s, const KArgs* a);

int moog_spec_configure(size_t lds) {
  int rc = moog_spec_configure_0(lds);
  if (!rc) rc = moog_spec_configure_1(lds);
  if (!rc) rc = moog_spec_configure_2(lds);
  return rc;
}

void moog_spec_launch(int n_envs, size_t lds, hipStream_t s, const KArgs* a) {
  if (a->traj[0].out) moog_spec_launch_2(n_envs, lds, s, a);   // (a trajectory is bound: a sequence, moog_engine.hip step_call)
  else if (a->repeat > 1 || a->reward_seq) moog_spec_launch_1(n_envs, lds, s, a);   // (a sequence of one step too: the one-step kernel knows nothing of KArgs::reward_seq)
  else moog_spec_launch_0(n_envs, lds, s, a);
}
#endif

}  // extern "C"
