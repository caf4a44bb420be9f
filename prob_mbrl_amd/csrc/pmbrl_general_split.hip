// General kernel family on split operands (pmbrl_gsplit.h: two fp16 pieces forward, two bf16 pieces in the
// adjoint): the instantiations of PM_GENERAL_SPLIT_INSTANCES and their table.
// (in-place form 3: the wide layers with every 512-wide stash pre-split for the dW GEMM -- pmbrl_dw_kernels.h,
//  pm_dw_wide_pre_kernel)
#include "pmbrl_host.h"
#include "pmbrl_mm.h"
#include "pmbrl_rollout.h"

#define PM_INST(RT, CA, CB, VAR, D, U, LD, NL, NT, TREE) \
  {reinterpret_cast<const void*>(&pm_rollout_fwd<RT, 2, VAR>), reinterpret_cast<const void*>(&pm_rollout_bwd<RT, 2, VAR>)},
static const PmInst fns[] = {PM_GENERAL_SPLIT_INSTANCES};
#undef PM_INST
static_assert(sizeof(fns) / sizeof(fns[0]) == pm_general_split_n, "one kernel pair per key");
PmInstTable pm_general_split_instances() { return {pm_general_split_keys, fns, pm_general_split_n}; }
