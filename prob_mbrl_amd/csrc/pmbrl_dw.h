// The records of the policy-gradient dW GEMM: what the plan (pmbrl_host.h) and the callers of its launchers hold.  The
// kernels are in pmbrl_dw_kernels.h, compiled into pmbrl_dw.hip only.  Nothing here needs the device compiler: the host-only
// planner (pmbrl_dw_plan.h) includes it.
#pragma once
#include <stdint.h>

#include "pmbrl.h"

#define PM_MAXL PMBRL_MAX_LAYERS      // (as pmbrl_dev.h)

#define PM_DW_NW 8
#define PM_DW_NT (PM_DW_NW * 64)
#define PM_DW_TM 4
#define PM_DW_TN 7
#define PM_DW_MAXBLK 256
#define PM_DW_TN_S 4   // split-operand form: blocks of at most 4 x 4 tiles (see pm_dw_block_s)

struct DwBlock {      // one wave block
  int16_t layer, ot0, it0, n_ot, n_it, pad;
};
// one 256 x 128 output tile of a wide layer (pm_dw_wide_kernel)
struct DwUnit {
  int16_t layer, m0, n0, pad;      // first output feature / first input feature of the tile
};
#define PM_DWW_TM 128
#define PM_DWW_TN 128
#define PM_DWW_LDK 40
#define PM_DWW_STAGE ((PM_DWW_TM + PM_DWW_TN) * 2 * PM_DWW_LDK)      // 16-bit elements per stage
#define PM_DWW_LDS_BYTES (2 * PM_DWW_STAGE * 2)

struct DwArgs {
  int nl, nsplit, n_chunks, chunks_per_split;
  int RT, Rw, n_params;
  int part_stride;                       // floats between the partial vectors of two splits (n_params rounded up to 4)
  int dim[PM_MAXL + 1], nt[PM_MAXL + 1];
  int w_off[PM_MAXL], b_off[PM_MAXL];    // offsets in the flat parameter vector
  const float* actT[PM_MAXL];
  const float* gT[PM_MAXL];
  const int* nvalid;                     // forward status word: only chunks of steps t < *nvalid exist (nullptr: all)
  int chunks_per_step;                   // nwg * RT
  const DwBlock* blocks;                 // sorted by wave
  int wave_first[PM_DW_NW + 1];          // wave w owns blocks [wave_first[w], wave_first[w+1])
  float* part;                           // [nsplit][n_params]
  int split_prec;                        // 1: two bf16 pieces per operand on the bf16 matrix core (pm_dw_kernel_s)
  // Pipelined form (pmbrl_dw_plan.h: "dW GEMM behind the adjoint sweep"): the adjoint sweep runs as K launches over
  // descending step ranges and launch k of this GEMM covers the chunks of range k only, [c_begin, c_end),
  // dealt to the same nsplit partial rows every time; the first launch that owns a valid step writes its
  // row (zeros if the row got no chunk), the later ones add to it -- still one fixed order of additions.
  int pipe;                              // 0: one launch over all chunks (fields below unused)
  int pipe_k;                            // index of this launch, 0 = the highest steps
  int c_begin, c_end;                    // chunk range of this launch (c_end = the previous launch's c_begin)
  int rows_before;                       // partial rows the earlier launches own (the last launch has more)
  // Rebuilding form of the whole-layer kernel (pm_dw_layer_rc_kernel: behind a register-resident adjoint sweep, which
  // stashes no delta of the policy's second hidden layer; a call fills these, pm_dw_call_args).  RT = 1: chunk c is the
  // (step, workgroup) block c of every stash and of the activity words -- chunks_per_step is the sweep's nwg
  const unsigned* rc_abits;              // (nullptr: the classic form, the delta is fetched) the forward sweep's activity words of that layer: [chunk][sweep wave (4)][lane]
  const float* rc_head;                  // the adjoint pack's transposed head weights: [tile][2 blocks][lane][4]
  float rc_inv_keep;                     // 1 / keep of the layer's dropout
  int rc_D, rc_U;                        // state and action widths: which rows of a gT[l + 1] block a lane group holds
  // Streamed form of the rebuilding kernel (pmbrl_dw_plan.h: "the second hidden layer's dW GEMM BESIDE the adjoint
  // sweep").  The steps [st_cut, valid steps) go to st_wgs consumer workgroups (pm_dw_layer_st_kernel) that run NEXT TO the one-launch sweep, on
  // the CUs it leaves idle, and follow it step by step: of the three inputs only the head gradient comes from the adjoint
  // sweep, which publishes it as tagged granules (st_pub: [H][chunks per step][2 U][16] x {tag, 32 bits}, step t's tag
  // st_tag + t).  Consumer w owns partial row w; pm_dw_layer_rc_kernel then takes the steps below the cut, dealt to the
  // rows the reduction reads, and adds to the consumers' rows (pm_dw_range_st).  Only the layer's W / b columns of the
  // partial rows are concerned: the other kernels run as without it.
  int st_on;                             // 0: off (fields below unused)
  int st_cut, st_wgs;
  const unsigned long long* st_pub;
  unsigned st_tag;
  int* st_fail;                          // the adjoint sweep's failure word (status[1]): set when a wait for a granule gives up
  // Every step streamed (st_cut == 0): the flat columns [own_lo, own_hi) hold chunks in the consumers' rows only.  The
  // reduction adds rows [0, st_wgs) alone in the float4 columns that lie wholly inside (pm_dw_reduce), and the consumers
  // write zeros beyond their rows only at the range's unaligned edges.  Empty: every row of every column is written and read
  int own_lo, own_hi;
  // ... and the policy head with it (st_head; the layer behind the streamed one, at most 16 outputs): its only adjoint-side
  // input is the head gradient the consumers hold anyway, so they form its dW = g^T actT and db = sum g too, with fp32 MFMAs
  // on register operands, and write them into their own partial rows; the block kernel then walks a table without the head
  // (pm_dw_kernel_nh) and [own_lo, own_hi) runs through the head's bias
  int st_head;
};
static_assert(sizeof(DwArgs) == 472, "DwArgs is a kernel argument: its layout does not move");
// LDS of the streamed consumer behind the stages: the policy head's table and accumulators (pmbrl_dw_kernels.h, PM_DWH_TAB)
#define PM_DWH_LDS_BYTES ((2 * 16 * 16 + PM_DW_NW * 64 * 12) * 4)

// tile sizes of the kernels of whole layers, which the plan's choice of them reads (pmbrl_dw_kernels.h)
#define PM_DWP_TM 256
#define PM_DWP_TN 256
#define PM_DWL_NT 13
