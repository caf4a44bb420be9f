// The layer-norm instances of the stand-alone network kernels (pmbrl_mlp.h: pm_mlp_fwd_kernel<true>,
// pm_mlp_bwdx_kernel<true>, pm_mlp_bwdp_kernel<*, true>) and their launches.  An object of their own: pmbrl_mlp.o then holds
// exactly the kernels it held before layer norm, instruction for instruction (tools/kernel_diff.py), and the two compile
// side by side.  The marshalling and the argument checks are pmbrl_mlp.hip's.
#include <hip/hip_runtime.h>

#include "pmbrl_host.h"
#include "pmbrl_mm.h"
#include "pmbrl_rollout.h"
#include "pmbrl_mlp.h"

int pm_mlp_ln_launch_fwd(hipStream_t s, int n_blocks, size_t lds, const MlpLnFwdArgs& a) {
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_mlp_fwd_kernel<true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(pm_mlp_fwd_kernel<true>, dim3(n_blocks), dim3(PM_NT), lds, s, a);
  HIPCHK(hipGetLastError());
  return 0;
}

int pm_mlp_ln_launch_bwdx(hipStream_t s, int n_blocks, size_t lds, const MlpLnBwdArgs& a) {
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_mlp_bwdx_kernel<true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(pm_mlp_bwdx_kernel<true>, dim3(n_blocks), dim3(PM_NT), lds, s, a);
  HIPCHK(hipGetLastError());
  return 0;
}

int pm_mlp_ln_launch_bwdp(hipStream_t s, int n_blocks, size_t lds, const MlpBwdLArgs& a, bool conc) {
  if (conc) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_mlp_bwdp_kernel<true, true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((pm_mlp_bwdp_kernel<true, true>), dim3(n_blocks), dim3(PM_NT), lds, s, a);
  } else {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_mlp_bwdp_kernel<false, true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((pm_mlp_bwdp_kernel<false, true>), dim3(n_blocks), dim3(PM_NT), lds, s, a);
  }
  HIPCHK(hipGetLastError());
  return 0;
}
