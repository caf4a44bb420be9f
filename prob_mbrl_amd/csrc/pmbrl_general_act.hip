// General kernel family for plans with a hidden layer that is not ReLU (PMBRL_ACT_TANH .. PMBRL_ACT_NONE, per layer;
// pmbrl_rollout.h: the ACT instances of pm_rollout_fwd / pm_rollout_bwd, EpiActFwdT / EpiActBwdT): the instantiations of
// PM_GENERAL_ACT_INSTANCES -- exact fp32 and split operands (two fp16 pieces forward, two bf16 pieces in the adjoint) --
// and their table.  Two activation buffers always: the in-place and wide layers stay ReLU-only.
#include "pmbrl_host.h"
#include "pmbrl_mm.h"
#include "pmbrl_rollout.h"

#define PM_INST(RT, CA, CB, VAR, D, U, LD, NL, NT, TREE)                \
  {reinterpret_cast<const void*>(&pm_rollout_fwd<RT, VAR, 0, true>), \
   reinterpret_cast<const void*>(&pm_rollout_bwd<RT, VAR, 0, true>)},
static const PmInst fns[] = {PM_GENERAL_ACT_INSTANCES};
#undef PM_INST
static_assert(sizeof(fns) / sizeof(fns[0]) == pm_general_act_n, "one kernel pair per key");
PmInstTable pm_general_act_instances() { return {pm_general_act_keys, fns, pm_general_act_n}; }
