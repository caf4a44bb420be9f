// The spill form of the BNN training step (pmbrl_bnn_spill.h): its four instances and their launcher, an object of their
// own -- pmbrl_bnn.o holds the kernels it always held.  The plan, the stashes' place in the workspace and the choice between
// the forms are pmbrl_bnn.hip's.
#include <hip/hip_runtime.h>

#include "pmbrl_host.h"
#include "pmbrl_mm.h"
#include "pmbrl_rollout.h"
#include "pmbrl_bnn_spill.h"

typedef void (*BnnSpillKernel)(const BnnSpillArgs);
static BnnSpillKernel bnn_spill_kernel(int act, int bern) {
  if (bern) return act ? pm_bnn_fwd_bwd_spill<true, true> : pm_bnn_fwd_bwd_spill<false, true>;
  return act ? pm_bnn_fwd_bwd_spill<true, false> : pm_bnn_fwd_bwd_spill<false, false>;
}

hipError_t pm_bnn_spill_prepare(int act, int bern) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(bnn_spill_kernel(act, bern)),
                             hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - PM_BNN_LDS_STATIC);
}

void pm_bnn_spill_launch(const BnnSpillArgs& A, int act, int bern, size_t lds_bytes, hipStream_t s) {
  hipLaunchKernelGGL(bnn_spill_kernel(act, bern), dim3(A.nwg), dim3(PM_NT), lds_bytes, s, A);
}
