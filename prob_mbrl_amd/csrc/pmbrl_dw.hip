// The policy-gradient dW GEMM (pmbrl_dw_kernels.h): its kernels, the wave blocks they walk, their LDS attributes and
// their launches.  Users: the rollout adjoint call (pmbrl.hip) and the BNN step (pmbrl_bnn.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <vector>

#include "pmbrl_host.h"
#include "pmbrl_dw_kernels.h"

// dW wave blocks: balanced splits of every layer's output tile grid into <= 4 x 7 tile
// blocks, dealt to the four SIMDs (waves w and w+4 share SIMD w) by decreasing size so that
// every SIMD issues the same number of MFMAs.  Returns the number of blocks; `blocks` comes back
// sorted by wave, wave w owning [wave_first[w], wave_first[w+1]).
// (ot_parts_min: a layer's output tiles in at least this many parts where it has as many -- the table without the policy
//  head, pm_dw_kernel_nh, has one layer left and wants a block on every wave)
int build_dw_blocks(int nl, const int* nt, std::vector<DwBlock>& blocks, int* wave_first, int tn_max,
                           const bool* skip, int ot_parts_min) {
  blocks.clear();
  auto split = [](int n, int maxsz, std::vector<std::pair<int, int>>& out, int parts_min = 1) {
    const int parts = std::max((n + maxsz - 1) / maxsz, std::min(n, parts_min));
    int lo = 0;
    for (int i = 0; i < parts; ++i) {
      const int sz = n / parts + (i < n % parts ? 1 : 0);
      out.push_back({lo, sz});
      lo += sz;
    }
  };
  for (int l = 0; l < nl; ++l) {
    if (skip && skip[l]) continue;      // a wide layer: pm_dw_wide_kernel
    std::vector<std::pair<int, int>> os, is;
    split(nt[l + 1], PM_DW_TM, os, ot_parts_min);
    split(nt[l], tn_max, is);
    for (auto& o : os)
      for (auto& i : is) {
        DwBlock b;
        b.layer = (int16_t)l;
        b.ot0 = (int16_t)o.first;
        b.n_ot = (int16_t)o.second;
        b.it0 = (int16_t)i.first;
        b.n_it = (int16_t)i.second;
        b.pad = 0;
        blocks.push_back(b);
      }
  }
  const int n_blocks = (int)blocks.size();
  // cost of a block = MFMAs per chunk in the shape class it runs in (see pm_dw_kernel)
  auto cost = [tn_max](const DwBlock& b) {
    const int ni = b.n_ot <= 1 ? 1 : (b.n_ot <= 3 ? 3 : 4);
    const int nj = b.n_it <= 1 ? 1 : (b.n_it <= 4 ? 4 : (b.n_it <= 6 ? 6 : 7));
    return ni * (tn_max <= 4 && nj > 1 ? 4 : nj);
  };
  std::stable_sort(blocks.begin(), blocks.end(),
                   [&](const DwBlock& a, const DwBlock& b) { return cost(a) > cost(b); });
  std::vector<DwBlock> per_wave[PM_DW_NW];
  long wave_load[PM_DW_NW] = {0};
  // waves w and w+4 of a workgroup share SIMD w (measured: pairing (2k, 2k+1) instead is 5% slower)
  for (const DwBlock& b : blocks) {
    int best_simd = 0;
    for (int sm = 1; sm < 4; ++sm)
      if (wave_load[sm] + wave_load[sm + 4] < wave_load[best_simd] + wave_load[best_simd + 4]) best_simd = sm;
    const int w = wave_load[best_simd] <= wave_load[best_simd + 4] ? best_simd : best_simd + 4;
    per_wave[w].push_back(b);
    wave_load[w] += cost(b);
  }
  blocks.clear();
  // the small blocks are latency-bound (a handful of MFMAs per chunk): the second wave of a SIMD runs
  // its FIRST, while the SIMD's other wave keeps the MFMA pipe busy with its big block
  for (int w = 0; w < PM_DW_NW; ++w) {
    wave_first[w] = (int)blocks.size();
    if (w >= 4) std::reverse(per_wave[w].begin(), per_wave[w].end());
    for (const DwBlock& b : per_wave[w]) blocks.push_back(b);
  }
  wave_first[PM_DW_NW] = (int)blocks.size();
  return n_blocks;
}

// dynamic LDS of the kernels plan_dw chose for this plan
int pm_dw_set_attr(const pmbrl_plan* p) {
  if (p->dw_layer13 >= 0) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_dw_layer_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, PM_DWL_LDS_BYTES));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_dw_layer_rc_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, PM_DWL_LDS_BYTES));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_dw_layer_st_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, PM_DWL_LDS_BYTES + PM_DWH_LDS_BYTES));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_dw_layer_rcb_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, PM_DWL_LDS_BYTES));
  }
  if (p->dw_pre_mask) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_dw_narrow_pre_kernel<1>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, PM_DWP_LDS_BYTES));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_dw_narrow_pre_kernel<2>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, PM_DWP_LDS_BYTES));
  }
  if (p->n_dw_units) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_dw_wide_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, PM_DWW_LDS_BYTES));
    if (p->dw_pre_mask)
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_dw_wide_pre_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, PM_DWP_LDS_BYTES));
  }
  return 0;
}

// ... of launch k of the pipelined form: the chunks of step range k, dealt to the partial rows of a grid next to the sweep
// (the last launch has the chip to itself)
static DwArgs dw_range_args(const pmbrl_plan* p, const DwArgs& W, int k) {
  DwArgs Wk = W;
  const int cps = W.chunks_per_step;
  Wk.pipe = 1;
  Wk.pipe_k = k;
  Wk.nsplit = k + 1 == p->pipe_K ? p->pipe_rows : p->pipe_grid;
  Wk.rows_before = p->pipe_grid;
  Wk.c_begin = p->pipe_lo[k] * cps;
  Wk.c_end = (k ? p->pipe_lo[k - 1] : p->cfg.H) * cps;
  Wk.chunks_per_split = (Wk.c_end - Wk.c_begin + Wk.nsplit - 1) / Wk.nsplit;
  if (p->dw_split) Wk.chunks_per_split = (Wk.chunks_per_split + 1) & ~1;
  return Wk;
}
// The dW GEMM over the chunks W describes, one partial row per workgroup: the only place that chooses its kernels.
// (The pipelined ranges never meet a plan without block-kernel layers or with pre-split stashes: such a plan has
//  dw_pre_mask -- the first layer's input is at most 40 wide, so only pm_dw_narrow_pre_kernel takes it from the block
//  kernel -- and plan_dw_pipe leaves the pipeline off for it.)
// (W.st_on, the streamed form: the layer's kernel is the launch behind the consumers -- it adds to their partial rows, so
//  `after`, the event behind them, is waited for in front of it; the other kernels neither read nor write those columns)
void pm_dw_launch(const pmbrl_plan* p, const DwArgs& W, hipStream_t s, hipEvent_t after) {
  const dim3 rows(W.nsplit), units((W.nsplit + 7) / 8 * 8 * p->n_dw_units);
  // (W.st_head: the consumers formed the head; the call's table is the one without it -- dw_call_args -- and where every
  //  block of that is at most 2 x 1 tiles, the kernel with the deeper ring walks it)
  assert(!W.st_head || !W.pipe);      // (pm_dw_kernel_nh has no branch for a row of zeros: only a piped range asks for one)
  if (W.st_head && p->n_dw_blocks_nh == 0) {}
  else if (W.st_head && p->dw_nh_ring) hipLaunchKernelGGL(pm_dw_kernel_nh, rows, dim3(PM_DW_NT), 0, s, W);
  else if (W.st_head) hipLaunchKernelGGL(pm_dw_kernel, rows, dim3(PM_DW_NT), 0, s, W);
  else if (p->n_dw_blocks == 0) {}      // (every layer has a GEMM kernel of its own: below)
  else if (p->dw_split) hipLaunchKernelGGL(pm_dw_kernel_s, rows, dim3(PM_DW_NT), 0, s, W);
  else hipLaunchKernelGGL(pm_dw_kernel, rows, dim3(PM_DW_NT), 0, s, W);
  if (p->dw_pre_mask)
    for (int l = 0; l < p->pol.nl; ++l) {
      if (!p->dw_narrow[l]) continue;
      const int g_wide = p->dw_narrow[l] == 1 ? 1 : 0, nt_n = g_wide ? p->pol.nt[l] : p->pol.nt[l + 1];
      if (nt_n <= 1) hipLaunchKernelGGL(pm_dw_narrow_pre_kernel<1>, rows, dim3(PM_DWP_NT), PM_DWP_LDS_BYTES, s, W, l, g_wide);
      else hipLaunchKernelGGL(pm_dw_narrow_pre_kernel<2>, rows, dim3(PM_DWP_NT), PM_DWP_LDS_BYTES, s, W, l, g_wide);
    }
  if (p->n_dw_units && p->dw_pre_mask)
    hipLaunchKernelGGL(pm_dw_wide_pre_kernel, units, dim3(PM_DWP_NT), PM_DWP_LDS_BYTES, s, W, p->dw_units_d, p->n_dw_units);
  else if (p->n_dw_units)
    hipLaunchKernelGGL(pm_dw_wide_kernel, units, dim3(PM_DW_NT), PM_DWW_LDS_BYTES, s, W, p->dw_units_d, p->n_dw_units);
  // (W carries what rebuilds the delta operand -- dw_call_args, behind a register-resident adjoint sweep, which left no
  //  stash of it: the rebuilding form.  It is written for 16-row chunks and the policy's second hidden layer, which is
  //  all pm_reg_can_run lets reach it)
  const bool rebuild = W.rc_abits != nullptr;
  assert(!rebuild || (W.RT == 1 && p->dw_layer13 == PM_REG_DW_LAYER));
  assert(!W.st_on || rebuild);
  if (after) (void)hipStreamWaitEvent(s, after, 0);
  if (W.st_on && W.st_cut == 0) return;      // (every step streamed: the consumers wrote every row the reduction reads)
  if (p->dw_layer13 >= 0 && rebuild && W.st_on)
    hipLaunchKernelGGL(pm_dw_layer_rcb_kernel, rows, dim3(PM_DW_NT), PM_DWL_LDS_BYTES, s, W, p->dw_layer13);
  else if (p->dw_layer13 >= 0 && rebuild)
    hipLaunchKernelGGL(pm_dw_layer_rc_kernel, rows, dim3(PM_DW_NT), PM_DWL_LDS_BYTES, s, W, p->dw_layer13);
  else if (p->dw_layer13 >= 0)
    hipLaunchKernelGGL(pm_dw_layer_kernel, rows, dim3(PM_DW_NT), PM_DWL_LDS_BYTES, s, W, p->dw_layer13);
}
void pm_dw_launch_range(const pmbrl_plan* p, const DwArgs& W, int k, hipStream_t s) { pm_dw_launch(p, dw_range_args(p, W, k), s); }
// the streamed form's consumers (W.st_on): one workgroup per CU the adjoint sweep leaves idle, next to it
void pm_dw_stream_launch(const pmbrl_plan* p, const DwArgs& W, hipStream_t s) {
  assert(W.st_on && W.rc_abits && W.RT == 1 && p->dw_layer13 == PM_REG_DW_LAYER);
  hipLaunchKernelGGL(pm_dw_layer_st_kernel, dim3(W.st_wgs), dim3(PM_DW_NT), PM_DWL_LDS_BYTES + PM_DWH_LDS_BYTES, s, W,
                     p->dw_layer13);
}
// the block kernel alone, one partial row per workgroup: the BNN step's dW / db (its stashes have the same layout)
void pm_dw_blocks_launch(const DwArgs& W, hipStream_t s) {
  hipLaunchKernelGGL(pm_dw_kernel, dim3(W.nsplit), dim3(PM_DW_NT), 0, s, W);
}
