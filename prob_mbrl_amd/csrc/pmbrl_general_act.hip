// General kernel family for plans with a network that is not ReLU (pmbrl_mlp activations PMBRL_ACT_TANH / PMBRL_ACT_SILU;
// pmbrl_rollout.h: the ACT instances of pm_rollout_fwd / pm_rollout_bwd, EpiActFwdT / EpiActBwdT): instantiations in exact
// fp32 and on split operands (two fp16 pieces forward, two bf16 pieces in the adjoint), attribute setup and launch dispatch.
// Two activation buffers always: the in-place and wide layers stay ReLU-only.
#include "pmbrl_host.h"
#include "pmbrl_mm.h"
#include "pmbrl_rollout.h"

template <int RT, int PR>
static int set_attr_act(size_t lds) {
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_rollout_fwd<RT, PR, 0, true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_rollout_bwd<RT, PR, 0, true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return 0;
}
template <int PR>
static int set_attr_rt(const pmbrl_plan* p) {
  switch (p->RT) {
    case 1: return set_attr_act<1, PR>(p->lds_bytes);
    case 2: return set_attr_act<2, PR>(p->lds_bytes);
    default: return set_attr_act<4, PR>(p->lds_bytes);
  }
}
int pm_general_act_set_attr(const pmbrl_plan* p) { return p->prec ? set_attr_rt<2>(p) : set_attr_rt<0>(p); }

template <int RT, int PR>
static void launch_act(const pmbrl_plan* p, const RolloutArgs& A, hipStream_t s, bool fwd) {
  if (fwd) hipLaunchKernelGGL((pm_rollout_fwd<RT, PR, 0, true>), dim3(p->nwg), dim3(PM_NT), p->lds_bytes, s, A);
  else hipLaunchKernelGGL((pm_rollout_bwd<RT, PR, 0, true>), dim3(p->nwg), dim3(PM_NT), p->lds_bytes, s, A);
}
template <int PR>
static void launch_rt(const pmbrl_plan* p, const RolloutArgs& A, hipStream_t s, bool fwd) {
  switch (p->RT) {
    case 1: launch_act<1, PR>(p, A, s, fwd); break;
    case 2: launch_act<2, PR>(p, A, s, fwd); break;
    default: launch_act<4, PR>(p, A, s, fwd); break;
  }
}
void pm_general_act_launch(const pmbrl_plan* p, const RolloutArgs& A, hipStream_t s, bool fwd) {
  if (p->prec) launch_rt<2>(p, A, s, fwd);
  else launch_rt<0>(p, A, s, fwd);
}
