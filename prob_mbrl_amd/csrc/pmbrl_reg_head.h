// What the register-resident adjoint sweep (pmbrl_reg.h, head_adjoint) and the dW GEMM that rebuilds the sweep's product
// (pmbrl_dw_kernels.h, the RC form of pm_dw_layer_kernel) share: the family's tile constants, its inline-asm MFMAs and the
// B fragments of the head's transposed product.  ONE definition of each: the rebuilt delta of the policy's second hidden
// layer is the sweep's own, bit for bit, only as long as both run the same instructions on the same operand bytes.
#pragma once
#include "pmbrl_dev.h"
#include "pmbrl_split.h"

#define PR_NW 4                 // waves per workgroup: one per SIMD
#define PR_SLOTS 3              // register-resident tiles per wave and hidden->hidden layer: tile 4 s + w
#define PR_XT 12                // the tile that lives in LDS (run by wave pr_xwave(net))
#define PR_FRAG 256             // floats of one fragment (64 lanes x 16 bytes)
typedef unsigned pr_u32x4 __attribute__((ext_vector_type(4)));

// the wave that runs the LDS-resident tile of a network (two different ones: they balance over a step)
__host__ __device__ constexpr int pr_xwave(int net) { return net; }

// ---------------------------------------------------------------------------
// MFMA with the A operand (weights) in the accumulator file or in a VGPR.  Inline asm: the compiler schedules the
// statement as one opaque instruction and pads nothing around it -- pr_mfma_fence() supplies the wait states
// between a chain's last MFMA and the first VALU read of its accumulator (8-pass XDL: 12 states), pr_mfma_open()
// those between a VALU write of an operand and the first MFMA of a group.
// ---------------------------------------------------------------------------
// NOP: two wait states in front of the instruction, INSIDE the statement.  A VGPR written by a VALU instruction may
// not be read as an MFMA operand in the next two issue slots (hipcc pads that for its own MFMAs, not for asm), and
// the compiler is free to schedule the VALU that builds an operand -- a cvt_pk of a fragment -- right in front of
// the statement that consumes it: measured as garbage head / tail products before this was here.  The big hidden
// layers need none (B operands come from ds_read, weights from the prologue).
template <bool F16, bool AG, bool NOP = false>
__device__ __forceinline__ void pr_mfma(f32x4& acc, const f32x4& w, const f32x4& b) {
  if constexpr (NOP) {
    if constexpr (F16) asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(b));
    else asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(b));
  } else if constexpr (F16) {
    if constexpr (AG) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(b));
    else asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(b));
  } else {
    if constexpr (AG) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(b));
    else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(b));
  }
}
// first product of a chain: C = 0 (inline constant), the accumulator is a pure output
template <bool F16, bool AG, bool NOP = false>
__device__ __forceinline__ void pr_mfma0(f32x4& acc, const f32x4& w, const f32x4& b) {
  if constexpr (NOP) {
    if constexpr (F16) asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(acc) : "v"(w), "v"(b));
    else asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(w), "v"(b));
  } else if constexpr (F16) {
    if constexpr (AG) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(acc) : "a"(w), "v"(b));
    else asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(acc) : "v"(w), "v"(b));
  } else {
    if constexpr (AG) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(acc) : "a"(w), "v"(b));
    else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(w), "v"(b));
  }
}
__device__ __forceinline__ void pr_mfma_open() { asm volatile("s_nop 3"); }
__device__ __forceinline__ void pr_mfma_fence() { asm volatile("s_nop 7\n\ts_nop 7"); }

// B fragments of a head's transposed product (the adjoint pack's PR_OFF_L0 section is the A operand: block 0 the means'
// rows, block 1 the log-stds'): gm / gl = float[2], the head gradient of the lane's two input slots, split into two bf16
// pieces; K slots 3 s + {0, 1, 2} = g.hi, g.lo, g.hi against the pack's W.hi, W.hi, W.lo.  bf = f32x4[2]: [0] the means,
// [1] the log-stds.  (A macro, not a function: as a function -- array references or values -- the sweep's twenty
// instances selected other instructions for the packing and spilled other scalar registers; expanded in place the
// sweep compiles to what it was, which is what its register budget was tuned on.)
#define PR_HEAD_BFRAGS(gm, gl, bf)                                                                                  \
  _Pragma("unroll") for (int k = 0; k < 2; ++k) {                                                                   \
    unsigned short hh[2], hl[2];                                                                                    \
    _Pragma("unroll") for (int s = 0; s < 2; ++s) {                                                                 \
      const float v = k == 0 ? gm[s] : gl[s];                                                                       \
      const unsigned a = pm_pk_bf16(v, 0.f) & 0xffffu;                                                              \
      hh[s] = (unsigned short)a;                                                                                    \
      hl[s] = (unsigned short)(pm_pk_bf16(v - pm_bf_lo(a), 0.f) & 0xffffu);                                         \
    }                                                                                                               \
    const pr_u32x4 u = {(unsigned)hh[0] | ((unsigned)hl[0] << 16), (unsigned)hh[0] | ((unsigned)hh[1] << 16),       \
                        (unsigned)hl[1] | ((unsigned)hh[1] << 16), 0u};                                             \
    bf[k] = __builtin_bit_cast(f32x4, u);                                                                           \
  }
// a stashed activity nibble as the four {0, 1 / keep} multipliers of its tile's accumulator registers
__device__ __forceinline__ f32x4 pr_nibble_mult(unsigned nib, float inv_keep) {
  f32x4 m;
#pragma unroll
  for (int r = 0; r < 4; ++r)      // (bit r as 0 / ~0 by one signed bit-field extract, one AND: inv_keep or +0.f)
    m[r] = __uint_as_float(__float_as_uint(inv_keep) & (unsigned)__builtin_amdgcn_sbfe((int)nib, (unsigned)r, 1u));
  return m;
}
