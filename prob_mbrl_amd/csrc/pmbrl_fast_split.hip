// Latency-optimised sweep kernels on split bf16 / fp16 operands (pmbrl_split.h): the instantiations of
// PM_SPLIT1_INSTANCES / PM_SPLIT2_INSTANCES and their table.  Compiled once per precision: -DPM_SPLIT_PR=1 (three bf16
// pieces forward) and -DPM_SPLIT_PR=2 (two fp16 pieces forward); the adjoint uses two bf16 pieces in both.
#include <type_traits>
#include "pmbrl_host.h"
#include "pmbrl_mm.h"
#include "pmbrl_rollout.h"
#include "pmbrl_fast.h"

#if !defined(PM_SPLIT_PR) || (PM_SPLIT_PR != 1 && PM_SPLIT_PR != 2)
#error "compile with -DPM_SPLIT_PR=1 or 2"
#endif

template <int D, int U, int LD, int NL, int NT, int TREE>
using Shape = std::conditional_t<TREE != 0, PfShapeTree<D, U, LD, NL, NT>, PfShape<D, U, LD, NL, NT>>;
#define PM_INST(RT, CA, CB, VAR, D, U, LD, NL, NT, TREE)                                                                   \
  {reinterpret_cast<const void*>(&pm_rollout_fwd_fast<RT, CA, CB, VAR, Shape<D, U, LD, NL, NT, TREE>, PM_SPLIT_PR>), \
   reinterpret_cast<const void*>(&pm_rollout_bwd_fast<RT, CA, CB, VAR, Shape<D, U, LD, NL, NT, TREE>, PM_SPLIT_PR>)},
#if PM_SPLIT_PR == 2
static const PmInst fns[] = {PM_SPLIT2_INSTANCES};
static_assert(sizeof(fns) / sizeof(fns[0]) == pm_fast_split2_n, "one kernel pair per key");
PmInstTable pm_fast_split2_instances() { return {pm_fast_split2_keys, fns, pm_fast_split2_n}; }
#else
static const PmInst fns[] = {PM_SPLIT1_INSTANCES};
static_assert(sizeof(fns) / sizeof(fns[0]) == pm_fast_split1_n, "one kernel pair per key");
PmInstTable pm_fast_split1_instances() { return {pm_fast_split1_keys, fns, pm_fast_split1_n}; }
#endif
#undef PM_INST
