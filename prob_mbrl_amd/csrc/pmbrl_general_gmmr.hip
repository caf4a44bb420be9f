// General kernel family for plans with a learned reward head on the mixture head (PMBRL_REWARD_LEARNED with
// dyn_components > 1; pmbrl_rollout.h: pm_rollout_fwd_gmmr / pm_rollout_bwd_gmmr, pmbrl_rollout_sweeps.h with PM_SWEEP_LR 1).  Kernels
// of their own, so that the instances every other plan resolves are the instructions they were.  Compiled once for ReLU
// networks (PM_GMMR_ACT=0) and once for networks with a hidden layer that is not ReLU (PM_GMMR_ACT=1), one object each;
// keyed like the ACT instances: row tiles, and piece planes (0: exact fp32, 2: split operands).  Two activation buffers
// always.
#include "pmbrl_host.h"
#include "pmbrl_mm.h"
#include "pmbrl_rollout.h"

#define PM_INST(RT, CA, CB, VAR, D, U, LD, NL, NT, TREE)                            \
  {reinterpret_cast<const void*>(&pm_rollout_fwd_gmmr<RT, VAR, 0, PM_GMMR_ACT != 0>), \
   reinterpret_cast<const void*>(&pm_rollout_bwd_gmmr<RT, VAR, 0, PM_GMMR_ACT != 0>)},
static const PmInst fns[] = {PM_GENERAL_ACT_INSTANCES};
#undef PM_INST
static_assert(sizeof(fns) / sizeof(fns[0]) == pm_general_act_n, "one kernel pair per key");
#if PM_GMMR_ACT
PmInstTable pm_general_gmmr_act_instances() { return {pm_general_act_keys, fns, pm_general_act_n}; }
#else
PmInstTable pm_general_gmmr_instances() { return {pm_general_act_keys, fns, pm_general_act_n}; }
#endif
