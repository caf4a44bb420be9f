// Latency-optimised sweep kernels, exact fp32 MFMA: the instantiations of PM_FAST_F32_INSTANCES and their table.
#include "pmbrl_host.h"
#include "pmbrl_mm.h"
#include "pmbrl_rollout.h"
#include "pmbrl_fast.h"

#define PM_INST(RT, CA, CB, VAR, D, U, LD, NL, NT, TREE)                                              \
  {reinterpret_cast<const void*>(&pm_rollout_fwd_fast<RT, CA, CB, VAR, PfShape<D, U, LD, NL, NT>>), \
   reinterpret_cast<const void*>(&pm_rollout_bwd_fast<RT, CA, CB, VAR, PfShape<D, U, LD, NL, NT>>)},
static const PmInst fns[] = {PM_FAST_F32_INSTANCES};
#undef PM_INST
static_assert(sizeof(fns) / sizeof(fns[0]) == pm_fast_f32_n, "one kernel pair per key");
PmInstTable pm_fast_f32_instances() { return {pm_fast_f32_keys, fns, pm_fast_f32_n}; }

// Outside the list, and no plan can select them: the barrier form of two stage pairs that 16-row workgroups do not have
// in this arithmetic.  The occupancy query that the table replaced instantiated them once per listed case, whatever its
// row tiles; they stay compiled until a change that is allowed to alter the set of instances.
#define PM_UNLISTED_MMG(CA, CB)                                                            \
  template __global__ void pm_rollout_fwd_fast<1, CA, CB, PF_VAR_MMG>(const RolloutArgs); \
  template __global__ void pm_rollout_bwd_fast<1, CA, CB, PF_VAR_MMG>(const RolloutArgs);
PM_UNLISTED_MMG(4, 3) PM_UNLISTED_MMG(1, 1)
#undef PM_UNLISTED_MMG
