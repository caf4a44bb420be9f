// The policy-gradient dW GEMM (pmbrl_dw_kernels.h): its kernels, their LDS attributes, the rollout plan's dW record made
// from the planner's decisions (pmbrl_dw_plan.h) and released, a call's argument record and the launches, which walk
// the record.  Users: the rollout adjoint call (pmbrl.hip) and the BNN step (pmbrl_bnn.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <vector>

#include "pmbrl_host.h"
#include "pmbrl_dw_kernels.h"

// dynamic LDS of the kernels the planner chose for this plan
static int pm_dw_set_attr(const DwPlan& D) {
  const bool layer = D.layer13 >= 0, pre = D.pre_mask != 0, units = D.unit_k != DwKernel::None;
  const struct { bool on; const void* fn; int bytes; } K[] = {
      {layer, reinterpret_cast<const void*>(&pm_dw_layer_kernel), PM_DWL_LDS_BYTES},
      {layer, reinterpret_cast<const void*>(&pm_dw_layer_rc_kernel), PM_DWL_LDS_BYTES},
      {layer, reinterpret_cast<const void*>(&pm_dw_layer_st_kernel), PM_DWL_LDS_BYTES + PM_DWH_LDS_BYTES},
      {layer, reinterpret_cast<const void*>(&pm_dw_layer_rcb_kernel), PM_DWL_LDS_BYTES},
      {pre, reinterpret_cast<const void*>(&pm_dw_narrow_pre_kernel<1>), PM_DWP_LDS_BYTES},
      {pre, reinterpret_cast<const void*>(&pm_dw_narrow_pre_kernel<2>), PM_DWP_LDS_BYTES},
      {units, reinterpret_cast<const void*>(&pm_dw_wide_kernel), PM_DWW_LDS_BYTES},
      {D.unit_k == DwKernel::WidePre, reinterpret_cast<const void*>(&pm_dw_wide_pre_kernel), PM_DWP_LDS_BYTES}};
  for (const auto& k : K)
    if (k.on) HIPCHK(hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes));
  return 0;
}

// table -> device -> DwArgs::blocks / wave_first, for the rollout plan's two tables and the BNN step's
hipError_t pm_dw_upload_blocks(const std::vector<DwBlock>& blocks, DwBlock** out) {
  *out = nullptr;
  hipError_t e = hipMalloc(out, std::max<size_t>(1, blocks.size()) * sizeof(DwBlock));
  if (e == hipSuccess && !blocks.empty()) e = hipMemcpy(*out, blocks.data(), blocks.size() * sizeof(DwBlock), hipMemcpyHostToDevice);
  if (e != hipSuccess && *out) { (void)hipFree(*out); *out = nullptr; }
  return e;
}
void pm_dw_bind_blocks(DwArgs& W, const DwBlock* blocks_d, const int* wave_first) {
  W.blocks = blocks_d;
  for (int w = 0; w <= PM_DW_NW; ++w) W.wave_first[w] = wave_first[w];
}

// The plan's dW record: what the planner reads of the plan, its decisions, then what they need on the device -- the unit
// list, the block tables, the kernels' attributes, the second stream and its events.  pm_dw_plan_destroy releases them
// (pmbrl_plan_destroy; a plan that failed half-way too).
int pm_dw_plan_create(pmbrl_plan* p, int cus) {
  DwShape S{};
  S.nl = p->pol.nl;
  for (int i = 0; i <= S.nl; ++i) { S.nt[i] = p->pol.nt[i]; S.dim[i] = p->pol.dim[i]; }
  for (int l = 0; l < S.nl; ++l) { S.w_off[l] = (int)p->pol.w_off[l]; S.b_off[l] = (int)p->pol.b_off[l]; }
  S.n_params = (int)p->pol.n_params; S.dyn_n_params = (int)p->dyn.n_params;
  S.prec = p->prec; S.RT = p->RT; S.fast = p->fast; S.inplace = p->inplace; S.nwg = p->nwg;
  S.H = p->cfg.H; S.U = p->cfg.U; S.cus = cus;
  S.whole = sweep_form(p) == SweepForm::Whole;
  S.mm_parts = p->mm_parts; S.reg = p->reg; S.reg_mm = p->reg_mm; S.reg_bwd = p->sw.reg_bwd;
  S.sw = p->sw;
  DwPlan& D = p->dw;
  pm_dw_plan(S, D);
  if (!D.units.empty()) {
    HIPCHK(hipMalloc(&D.units_d, D.units.size() * sizeof(DwUnit)));
    HIPCHK(hipMemcpy(D.units_d, D.units.data(), D.units.size() * sizeof(DwUnit), hipMemcpyHostToDevice));
  }
  if (int rc = pm_dw_set_attr(D)) return rc;
  DwBlock* blocks_d = nullptr;
  HIPCHK(pm_dw_upload_blocks(D.blocks, &blocks_d));
  D.args.blocks = blocks_d;
  if (D.pipe_K > 1 || D.st_on) {
    HIPCHK(hipStreamCreateWithFlags(&D.pipe_stream, hipStreamNonBlocking));
    for (int k = 0; k < std::max(D.pipe_K, D.st_on ? 2 : 0); ++k)
      HIPCHK(hipEventCreateWithFlags(&D.pipe_ev[k], hipEventDisableTiming));
  }
  // (a table that cannot be had is no reason to fail the plan: the head stays in the block kernel)
  if (D.st_head && pm_dw_upload_blocks(D.blocks_nh, &D.blocks_nh_d) != hipSuccess) {
    (void)hipGetLastError();
    D.st_head = 0;
    D.table_nh_k = DwKernel::None;
  }
  return 0;
}
void pm_dw_plan_destroy(pmbrl_plan* p) {
  DwPlan& D = p->dw;
  if (D.args.blocks) (void)hipFree(const_cast<DwBlock*>(D.args.blocks));
  if (D.blocks_nh_d) (void)hipFree(D.blocks_nh_d);
  if (D.units_d) (void)hipFree(D.units_d);
  if (D.pipe_stream) (void)hipStreamDestroy(D.pipe_stream);
  for (int k = 0; k < PM_PIPE_MAX; ++k)
    if (D.pipe_ev[k]) (void)hipEventDestroy(D.pipe_ev[k]);
}

// the dW GEMM's arguments: the plan's part (DwPlan::args) + this call's stashes, partial rows and status word
DwArgs pm_dw_call_args(const pmbrl_plan* p, void* workspace, int32_t* status, const RolloutArgs& A, bool rebuilt, bool streamed) {
  const DwPlan& D = p->dw;
  DwArgs W = D.args;
  if (streamed) {
    // the streamed form of the layer's GEMM: the granules the sweep of THIS call publishes, under its launch generation
    // (generation + step + 1, never 0: xch_prepare's rule)
    W.st_on = 1;
    W.st_cut = D.st_cut;
    W.st_wgs = D.st_wgs;
    W.st_pub = reinterpret_cast<const unsigned long long*>(static_cast<char*>(workspace) + D.off_pub);
    W.st_tag = ((++D.pub_gen) << 12) + 1u;
    W.st_fail = status ? status + 1 : nullptr;
    if (W.st_cut == 0) {
      // every step streamed: the layer's columns (W then b, one contiguous range of the flat vector) hold chunks in the
      // consumers' rows only -- what the consumers need not zero and the reduction need not read
      const int l = D.layer13;
      if (W.b_off[l] == W.w_off[l] + W.dim[l + 1] * W.dim[l]) {
        W.own_lo = W.w_off[l];
        W.own_hi = W.b_off[l] + W.dim[l + 1];
      }
      if (D.st_head) {
        // ... and the head's (pm_dw_plan_head: contiguous behind the layer's); the block kernel's table is the one without it
        W.st_head = 1;
        W.own_hi = W.b_off[l + 1] + W.dim[l + 2];
        pm_dw_bind_blocks(W, D.blocks_nh_d, D.wave_first_nh);
      }
    }
  }
  for (int l = 0; l < p->pol.nl; ++l) { W.actT[l] = A.actT[l]; W.gT[l] = A.gT[l]; }
  W.part = reinterpret_cast<float*>(static_cast<char*>(workspace) + D.off_part);
  W.nvalid = status;
  // (the rebuilding form is written for 16-row chunks and the policy's second hidden layer, which is all pm_reg_can_run
  //  lets reach it; the streamed form is one of it)
  assert(!rebuilt || (W.RT == 1 && D.layer13 == PM_REG_DW_LAYER));
  assert(!streamed || rebuilt);
  if (rebuilt) {      // (gT[1] does not exist: the layer kernel rebuilds it)
    pm_reg_dw_rebuild_args(p, static_cast<char*>(workspace), W);
    W.rc_inv_keep = A.pol.inv_keep[1];
  }
  return W;
}
// ... of launch k of the pipelined form: the chunks of step range k, dealt to the partial rows of a grid next to the sweep
// (the last launch has the chip to itself)
static DwArgs dw_range_args(const DwPlan& D, const DwArgs& W, int k, int H) {
  DwArgs Wk = W;
  const int cps = W.chunks_per_step;
  Wk.pipe = 1;
  Wk.pipe_k = k;
  Wk.nsplit = k + 1 == D.pipe_K ? D.pipe_rows : D.pipe_grid;
  Wk.rows_before = D.pipe_grid;
  Wk.c_begin = D.pipe_lo[k] * cps;
  Wk.c_end = (k ? D.pipe_lo[k - 1] : H) * cps;
  Wk.chunks_per_split = (Wk.c_end - Wk.c_begin + Wk.nsplit - 1) / Wk.nsplit;
  if (W.split_prec) Wk.chunks_per_split = (Wk.chunks_per_split + 1) & ~1;
  return Wk;
}
// The dW GEMM over the chunks W describes, one partial row per workgroup: a straight walk over the kernels the planner
// resolved (DwPlan::table_k / table_nh_k, layer_k, unit_k, layer13).  Of the call it reads three facts, all in W: the
// head in the consumers (st_head: the call's table is the one without it, pm_dw_call_args), streamed (st_on), the
// delta rebuilt or fetched (rc_abits).
// (W.st_on, the streamed form: the layer's kernel is the launch behind the consumers -- it adds to their partial rows, so
//  `after`, the event behind them, is waited for in front of it; the other kernels neither read nor write those columns)
void pm_dw_launch(const pmbrl_plan* p, const DwArgs& W, hipStream_t s, hipEvent_t after) {
  const DwPlan& D = p->dw;
  const int n_units = (int)D.units.size();
  const dim3 rows(W.nsplit), units((W.nsplit + 7) / 8 * 8 * n_units);
  switch (W.st_head ? D.table_nh_k : D.table_k) {
    case DwKernel::Block: hipLaunchKernelGGL(pm_dw_kernel, rows, dim3(PM_DW_NT), 0, s, W); break;
    case DwKernel::BlockSplit: hipLaunchKernelGGL(pm_dw_kernel_s, rows, dim3(PM_DW_NT), 0, s, W); break;
    case DwKernel::BlockRing: hipLaunchKernelGGL(pm_dw_kernel_nh, rows, dim3(PM_DW_NT), 0, s, W); break;
    default: break;      // (every layer has a GEMM kernel of its own: below)
  }
  for (int l = 0; l < W.nl; ++l) {
    const int g_wide = D.narrow[l] == 1 ? 1 : 0;
    if (D.layer_k[l] == DwKernel::NarrowPre1)
      hipLaunchKernelGGL(pm_dw_narrow_pre_kernel<1>, rows, dim3(PM_DWP_NT), PM_DWP_LDS_BYTES, s, W, l, g_wide);
    else if (D.layer_k[l] == DwKernel::NarrowPre2)
      hipLaunchKernelGGL(pm_dw_narrow_pre_kernel<2>, rows, dim3(PM_DWP_NT), PM_DWP_LDS_BYTES, s, W, l, g_wide);
  }
  if (D.unit_k == DwKernel::WidePre)
    hipLaunchKernelGGL(pm_dw_wide_pre_kernel, units, dim3(PM_DWP_NT), PM_DWP_LDS_BYTES, s, W, D.units_d, n_units);
  else if (D.unit_k == DwKernel::Wide)
    hipLaunchKernelGGL(pm_dw_wide_kernel, units, dim3(PM_DW_NT), PM_DWW_LDS_BYTES, s, W, D.units_d, n_units);
  if (after) (void)hipStreamWaitEvent(s, after, 0);
  if (W.st_on && W.st_cut == 0) return;      // (every step streamed: the consumers wrote every row the reduction reads)
  if (D.layer13 < 0) return;
  // (W carries what rebuilds the delta operand -- pm_dw_call_args, behind a register-resident adjoint sweep, which left no
  //  stash of it: the rebuilding form)
  if (W.st_on) hipLaunchKernelGGL(pm_dw_layer_rcb_kernel, rows, dim3(PM_DW_NT), PM_DWL_LDS_BYTES, s, W, D.layer13);
  else if (W.rc_abits) hipLaunchKernelGGL(pm_dw_layer_rc_kernel, rows, dim3(PM_DW_NT), PM_DWL_LDS_BYTES, s, W, D.layer13);
  else hipLaunchKernelGGL(pm_dw_layer_kernel, rows, dim3(PM_DW_NT), PM_DWL_LDS_BYTES, s, W, D.layer13);
}
void pm_dw_launch_range(const pmbrl_plan* p, const DwArgs& W, int k, hipStream_t s) { pm_dw_launch(p, dw_range_args(p->dw, W, k, p->cfg.H), s); }
// the streamed form's consumers (W.st_on): one workgroup per CU the adjoint sweep leaves idle, next to it
void pm_dw_stream_launch(const pmbrl_plan* p, const DwArgs& W, hipStream_t s) {
  assert(W.st_on && W.rc_abits);
  hipLaunchKernelGGL(pm_dw_layer_st_kernel, dim3(W.st_wgs), dim3(PM_DW_NT), PM_DWL_LDS_BYTES + PM_DWH_LDS_BYTES, s, W,
                     p->dw.layer13);
}
// the block kernel alone, one partial row per workgroup: the BNN step's dW / db (its stashes have the same layout)
void pm_dw_blocks_launch(const DwArgs& W, hipStream_t s) {
  hipLaunchKernelGGL(pm_dw_kernel, dim3(W.nsplit), dim3(PM_DW_NT), 0, s, W);
}
