// Stand-alone network evaluation (pmbrl_mlp.h): forward, input gradient and full backward of one MLP.  The layer-norm
// instances of the three kernels are compiled in pmbrl_mlp_ln.hip, so that this object holds the kernels it always held.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "pmbrl_host.h"
#include "pmbrl_mm.h"
#include "pmbrl_rollout.h"
#include "pmbrl_mlp.h"

// grad_params[i] = sum over the slabs, in slab order (pm_mlp_bwdp_kernel; a non-template kernel, so defined in this object)
__global__ void pm_mlp_bwd_reduce_kernel(const float* __restrict__ slab, int n_slab, size_t n_params,
                                         float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_params) return;
  float s = 0.f;
  for (int b = 0; b < n_slab; ++b) s += slab[(size_t)b * n_params + i];
  out[i] = s;
}

// ---------------------------------------------------------------------------
// stand-alone network evaluation
// ---------------------------------------------------------------------------
struct MlpLayout {
  int nl, LD, act;      // act: PMBRL_ACT_* per hidden layer (pm_act_layers)
  int dim[PM_MAXL + 1], nt[PM_MAXL + 1];
  size_t wf[PM_MAXL], wb[PM_MAXL], bias[PM_MAXL], w_off[PM_MAXL], b_off[PM_MAXL], bytes, lds, lds_bwd, lds_bwdp, n_params;
};
static int mlp_layout(const pmbrl_mlp_call* c, MlpLayout& L) {
  if (!c) return fail(-1, "null argument");
  const pmbrl_mlp& m = c->net;
  if (m.n_layers < 2 || m.n_layers > PM_MAXL) return fail(-2, "mlp: 2..8 layers");
  if (c->B < 1) return fail(-2, "mlp: B must be >= 1");
  if (m.dims[m.n_layers] % 2) return fail(-2, "mlp: the output layer must be 2 x n_out wide");
  L.nl = m.n_layers;
  int maxnt = 1;
  size_t off = 0, po = 0;
  for (int i = 0; i <= L.nl; ++i) {
    if (m.dims[i] < 1 || m.dims[i] > 16 * 64) return fail(-2, "mlp: layer width out of range");
    L.dim[i] = m.dims[i];
    L.nt[i] = (m.dims[i] + 15) / 16;
    maxnt = std::max(maxnt, L.nt[i]);
  }
  for (int l = 0; l < L.nl; ++l) {
    L.w_off[l] = po; po += (size_t)L.dim[l + 1] * L.dim[l];
    L.b_off[l] = po; po += (size_t)L.dim[l + 1];
    L.wf[l] = off; off += (size_t)L.nt[l + 1] * L.nt[l] * 256 * sizeof(float);
    L.wb[l] = off; off += (size_t)L.nt[l + 1] * L.nt[l] * 256 * sizeof(float);
    L.bias[l] = off; off += (size_t)L.nt[l + 1] * 16 * sizeof(float);
    if (l < L.nl - 1 && !(m.keep[l] > 0.f)) return fail(-2, "mlp: keep must be > 0");
  }
  L.bytes = off;
  L.n_params = po;
  L.LD = maxnt * 16 + 8;
  L.lds = (2 * (size_t)16 * L.LD + (size_t)PM_NW * PM_KS_NT * 256) * sizeof(float);
  if (const char* why = pm_act_refusal(c->act, L.nl - 1)) return fail(-2, std::string("mlp: ") + why);
  L.act = pm_act_layers(c->act, L.nl - 1);
  L.lds_bwd = pm_mlp_bwd_lds_floats(L.nl, L.LD, L.act) * sizeof(float);
  L.lds_bwdp = pm_mlp_bwdp_lds_floats(L.nl, L.LD, L.act) * sizeof(float);
  if (L.lds > 160 * 1024) return fail(-3, "mlp: network too wide for LDS");
  return 0;
}

extern "C" size_t pmbrl_mlp_workspace_bytes(const pmbrl_mlp_call* c) {
  MlpLayout L;
  return mlp_layout(c, L) ? 0 : L.bytes;
}

// the layer-norm layers of a pmbrl_mlp_*_ln call: which hidden layers, their zhat buffers (counted on from z0, the
// buffers in front of them) and where their [d gamma | d beta] sits in grad_ln
struct MlpLnLayout {
  int n_ln, z_idx[PM_MAXL];
  size_t g_off[PM_MAXL], n_gb;
};
static int mlp_ln_layout(const pmbrl_mlp_layer_norm* ln, const MlpLayout& L, int z0, MlpLnLayout& N) {
  N.n_ln = 0;
  N.n_gb = 0;
  for (int l = 0; l < PM_MAXL; ++l) {
    N.z_idx[l] = 0;
    N.g_off[l] = 0;
    if (!ln->gamma_d[l]) continue;
    if (l >= L.nl - 1) return fail(-2, "mlp layer norm: gamma_d given for a layer that is not a hidden layer");
    if (!ln->beta_d[l]) return fail(-1, "mlp layer norm: a layer with gamma_d needs beta_d");
    if (!(ln->eps[l] > 0.f)) return fail(-2, "mlp layer norm: eps must be > 0");
    N.z_idx[l] = z0 + N.n_ln++;
    N.g_off[l] = N.n_gb;
    N.n_gb += 2 * (size_t)L.dim[l + 1];
  }
  if (!N.n_ln) return fail(-2, "mlp layer norm: no layer-norm layer (pass NULL for a network without one)");
  return 0;
}
static void mlp_ln_args(const pmbrl_mlp_layer_norm* ln, const MlpLayout& L, const MlpLnLayout& N, MlpLnArgs& A) {
  memset(&A, 0, sizeof(A));
  for (int l = 0; l < L.nl - 1; ++l) {
    A.gamma[l] = ln->gamma_d[l];
    A.beta[l] = ln->beta_d[l];
    A.eps[l] = ln->eps[l];
    A.z_idx[l] = N.z_idx[l];
    A.g_off[l] = N.g_off[l];
  }
  A.n_ln = N.n_gb;
}

extern "C" size_t pmbrl_mlp_ln_workspace_bytes(const pmbrl_mlp_call* c, const pmbrl_mlp_layer_norm* ln) {
  MlpLayout L;
  MlpLnLayout N;
  if (mlp_layout(c, L)) return 0;
  if (ln && mlp_ln_layout(ln, L, 0, N)) return 0;
  return L.bytes;
}

// pmbrl_mlp_forward (ln == nullptr) and pmbrl_mlp_forward_ln: one marshalling, two kernels
static int mlp_forward_run(void* stream, const pmbrl_mlp_call* c, void* workspace_d,
                           const float* x_d, const float* params_flat_d,
                           const uint16_t* const* mask_bits_d, const float* z_d,
                           const float* in_shift_d, const float* in_iscale_d,
                           const float* out_scale_d, const float* out_shift_d,
                           const float* sq_scale_d, const float* sq_bias_d,
                           float* sample_d, float* mean_d, float* log_std_d, const pmbrl_mlp_layer_norm* ln) {
  MlpLayout L;
  MlpLnLayout N;
  int rc = mlp_layout(c, L);
  if (rc) return rc;
  if (ln && (rc = mlp_ln_layout(ln, L, 0, N))) return rc;
  if (!workspace_d || !x_d || !params_flat_d) return fail(-1, "null argument");
  if ((in_shift_d == nullptr) != (in_iscale_d == nullptr) || (out_scale_d == nullptr) != (out_shift_d == nullptr) ||
      (sq_scale_d == nullptr) != (sq_bias_d == nullptr))
    return fail(-1, "mlp: shift/scale pointers come in pairs");
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace_d);
  PackArgs PK;
  PK.wflag = nullptr;
  PK.gen = 0;
  PK.n = 0;
  PK.status = nullptr;
  MlpArgs A;
  memset(&A, 0, sizeof(A));
  A.B = c->B; A.nl = L.nl; A.LD = L.LD; A.n_out = L.dim[L.nl] / 2;
  for (int i = 0; i <= L.nl; ++i) { A.dim[i] = L.dim[i]; A.nt[i] = L.nt[i]; }
  for (int l = 0; l < L.nl; ++l) {
    float* wf = reinterpret_cast<float*>(ws + L.wf[l]);
    float* bs = reinterpret_cast<float*>(ws + L.bias[l]);
    PK.job[PK.n++] = PackJob{params_flat_d + L.w_off[l], wf, L.dim[l + 1], L.dim[l], 0, 1, 0, 0, 0};
    PK.job[PK.n++] = PackJob{params_flat_d + L.b_off[l], bs, L.dim[l + 1], L.dim[l], 0, 1, 1, 0, 0};
    A.wf[l] = wf;
    A.bias[l] = bs;
    A.mask[l] = (l < L.nl - 1 && mask_bits_d) ? mask_bits_d[l] : nullptr;
    A.keep[l] = l < L.nl - 1 ? c->net.keep[l] : 1.f;
  }
  A.x = x_d; A.z = z_d; A.in_shift = in_shift_d; A.in_iscale = in_iscale_d;
  A.out_scale = out_scale_d; A.out_shift = out_shift_d; A.sq_scale = sq_scale_d; A.sq_bias = sq_bias_d;
  A.mls = c->max_log_std;
  A.act = L.act;
  A.sample = sample_d; A.mean = mean_d; A.log_std = log_std_d;
  pm_pack_all_launch(PK, s);
  if (!ln) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_mlp_fwd_kernel<false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
    hipLaunchKernelGGL(pm_mlp_fwd_kernel<false>, dim3((c->B + 15) / 16), dim3(PM_NT), L.lds, s, A);
  } else {
    MlpLnFwdArgs F;
    static_cast<MlpArgs&>(F) = A;
    mlp_ln_args(ln, L, N, F.ln);
    return pm_mlp_ln_launch_fwd(s, (c->B + 15) / 16, L.lds, F);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int pmbrl_mlp_forward(void* stream, const pmbrl_mlp_call* c, void* workspace_d,
                                 const float* x_d, const float* params_flat_d,
                                 const uint16_t* const* mask_bits_d, const float* z_d,
                                 const float* in_shift_d, const float* in_iscale_d,
                                 const float* out_scale_d, const float* out_shift_d,
                                 const float* sq_scale_d, const float* sq_bias_d,
                                 float* sample_d, float* mean_d, float* log_std_d) {
  return mlp_forward_run(stream, c, workspace_d, x_d, params_flat_d, mask_bits_d, z_d, in_shift_d, in_iscale_d, out_scale_d,
                         out_shift_d, sq_scale_d, sq_bias_d, sample_d, mean_d, log_std_d, nullptr);
}

extern "C" int pmbrl_mlp_forward_ln(void* stream, const pmbrl_mlp_call* c, void* workspace_d,
                                    const float* x_d, const float* params_flat_d,
                                    const uint16_t* const* mask_bits_d, const float* z_d,
                                    const float* in_shift_d, const float* in_iscale_d,
                                    const float* out_scale_d, const float* out_shift_d,
                                    const float* sq_scale_d, const float* sq_bias_d,
                                    float* sample_d, float* mean_d, float* log_std_d, const pmbrl_mlp_layer_norm* ln) {
  return mlp_forward_run(stream, c, workspace_d, x_d, params_flat_d, mask_bits_d, z_d, in_shift_d, in_iscale_d, out_scale_d,
                         out_shift_d, sq_scale_d, sq_bias_d, sample_d, mean_d, log_std_d, ln);
}

// pmbrl_mlp_grad_input (ln == nullptr) and pmbrl_mlp_grad_input_ln
static int mlp_grad_input_run(void* stream, const pmbrl_mlp_call* c, void* workspace_d,
                              const float* x_d, const float* params_flat_d,
                              const uint16_t* const* mask_bits_d, const float* z_d,
                              const float* in_shift_d, const float* in_iscale_d,
                              const float* out_scale_d, const float* out_shift_d,
                              const float* sq_scale_d, const float* sq_bias_d,
                              const float* g_sample_d, const float* g_mean_d,
                              const float* g_log_std_d, float* grad_x_d, const pmbrl_mlp_layer_norm* ln) {
  MlpLayout L;
  MlpLnLayout N;
  int rc = mlp_layout(c, L);
  if (rc) return rc;
  if (ln) {
    if ((rc = mlp_ln_layout(ln, L, 0, N))) return rc;
    L.lds_bwd = pm_mlp_bwd_lds_floats(L.nl, L.LD, L.act, N.n_ln) * sizeof(float);
  }
  if (!workspace_d || !x_d || !params_flat_d || !grad_x_d) return fail(-1, "null argument");
  if (L.lds_bwd > 160 * 1024) return fail(-3, "mlp: network too wide / deep for the input-gradient kernel's LDS budget");
  if ((in_shift_d == nullptr) != (in_iscale_d == nullptr) || (out_scale_d == nullptr) != (out_shift_d == nullptr) ||
      (sq_scale_d == nullptr) != (sq_bias_d == nullptr))
    return fail(-1, "mlp: shift/scale pointers come in pairs");
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace_d);
  PackArgs PK;
  PK.wflag = nullptr;
  PK.gen = 0;
  PK.n = 0;
  PK.status = nullptr;
  MlpBwdArgs Bw;
  memset(&Bw, 0, sizeof(Bw));
  MlpArgs& A = Bw.f;
  A.B = c->B; A.nl = L.nl; A.LD = L.LD; A.n_out = L.dim[L.nl] / 2;
  for (int i = 0; i <= L.nl; ++i) { A.dim[i] = L.dim[i]; A.nt[i] = L.nt[i]; }
  for (int l = 0; l < L.nl; ++l) {
    float* wf = reinterpret_cast<float*>(ws + L.wf[l]);
    float* wb = reinterpret_cast<float*>(ws + L.wb[l]);
    float* bs = reinterpret_cast<float*>(ws + L.bias[l]);
    PK.job[PK.n++] = PackJob{params_flat_d + L.w_off[l], wf, L.dim[l + 1], L.dim[l], 0, 1, 0, 0, 0};
    PK.job[PK.n++] = PackJob{params_flat_d + L.w_off[l], wb, L.dim[l + 1], L.dim[l], 1, 1, 0, 0, 0};
    PK.job[PK.n++] = PackJob{params_flat_d + L.b_off[l], bs, L.dim[l + 1], L.dim[l], 0, 1, 1, 0, 0};
    A.wf[l] = wf; Bw.wb[l] = wb; A.bias[l] = bs;
    A.mask[l] = (l < L.nl - 1 && mask_bits_d) ? mask_bits_d[l] : nullptr;
    A.keep[l] = l < L.nl - 1 ? c->net.keep[l] : 1.f;
  }
  A.x = x_d; A.z = z_d; A.in_shift = in_shift_d; A.in_iscale = in_iscale_d;
  A.out_scale = out_scale_d; A.out_shift = out_shift_d; A.sq_scale = sq_scale_d; A.sq_bias = sq_bias_d;
  A.mls = c->max_log_std;
  A.act = L.act;
  Bw.g_sample = g_sample_d; Bw.g_mean = g_mean_d; Bw.g_log_std = g_log_std_d; Bw.grad_x = grad_x_d;
  pm_pack_all_launch(PK, s);
  if (ln) {
    MlpLnBwdArgs F;
    F.b = Bw;
    mlp_ln_args(ln, L, N, F.ln);
    return pm_mlp_ln_launch_bwdx(s, (c->B + 15) / 16, L.lds_bwd, F);
  } else {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_mlp_bwdx_kernel<false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds_bwd));
    hipLaunchKernelGGL(pm_mlp_bwdx_kernel<false>, dim3((c->B + 15) / 16), dim3(PM_NT), L.lds_bwd, s, Bw);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int pmbrl_mlp_grad_input(void* stream, const pmbrl_mlp_call* c, void* workspace_d,
                                    const float* x_d, const float* params_flat_d,
                                    const uint16_t* const* mask_bits_d, const float* z_d,
                                    const float* in_shift_d, const float* in_iscale_d,
                                    const float* out_scale_d, const float* out_shift_d,
                                    const float* sq_scale_d, const float* sq_bias_d,
                                    const float* g_sample_d, const float* g_mean_d,
                                    const float* g_log_std_d, float* grad_x_d) {
  return mlp_grad_input_run(stream, c, workspace_d, x_d, params_flat_d, mask_bits_d, z_d, in_shift_d, in_iscale_d,
                            out_scale_d, out_shift_d, sq_scale_d, sq_bias_d, g_sample_d, g_mean_d, g_log_std_d, grad_x_d,
                            nullptr);
}

extern "C" int pmbrl_mlp_grad_input_ln(void* stream, const pmbrl_mlp_call* c, void* workspace_d,
                                       const float* x_d, const float* params_flat_d,
                                       const uint16_t* const* mask_bits_d, const float* z_d,
                                       const float* in_shift_d, const float* in_iscale_d,
                                       const float* out_scale_d, const float* out_shift_d,
                                       const float* sq_scale_d, const float* sq_bias_d,
                                       const float* g_sample_d, const float* g_mean_d,
                                       const float* g_log_std_d, float* grad_x_d, const pmbrl_mlp_layer_norm* ln) {
  return mlp_grad_input_run(stream, c, workspace_d, x_d, params_flat_d, mask_bits_d, z_d, in_shift_d, in_iscale_d,
                            out_scale_d, out_shift_d, sq_scale_d, sq_bias_d, g_sample_d, g_mean_d, g_log_std_d, grad_x_d,
                            ln);
}


// ---------------------------------------------------------------------------
// backward with respect to the input rows AND the parameters (pm_mlp_bwdp_kernel)
// ---------------------------------------------------------------------------
// the layout of a backward call: the forward's, refused where the kernel's own LDS need (every Linear's input, and with
// Tanh / SiLU every hidden layer's derivatives, stay resident) exceeds the 160 KB of a CU
static int mlp_backward_layout(const pmbrl_mlp_call* c, MlpLayout& L) {
  int rc = mlp_layout(c, L);
  if (rc) return rc;
  if (L.lds_bwdp > 160 * 1024)
    return fail(-3, "mlp: network too wide / deep for the backward kernel's LDS budget (160 KB)");
  return 0;
}
// workgroups of the backward kernel = gradient slabs in the workspace
static int mlp_backward_blocks(const pmbrl_mlp_call* c, const MlpLayout& L) {
  const size_t slab = L.n_params * sizeof(float);
  const size_t fit = std::max<size_t>(1, PMBRL_MLP_BWD_SLAB_BYTES / slab);
  const size_t cap = std::min<size_t>(PMBRL_MLP_BWD_MAX_BLOCKS, fit);
  return (int)std::min<size_t>(cap, ((size_t)c->B + 15) / 16);
}
static size_t mlp_slab_offset(const MlpLayout& L) { return (L.bytes + 255) & ~(size_t)255; }

extern "C" size_t pmbrl_mlp_backward_workspace_bytes(const pmbrl_mlp_call* c) {
  MlpLayout L;
  if (mlp_backward_layout(c, L)) return 0;
  return mlp_slab_offset(L) + (size_t)mlp_backward_blocks(c, L) * L.n_params * sizeof(float);
}

static size_t mlp_logit_slab_offset(const pmbrl_mlp_call* c, const MlpLayout& L);
// the concrete-dropout layers of a pmbrl_mlp_backward_concrete call: which hidden layers, where their logits sit in the
// gradient, and the kernel's LDS need with one Q buffer per such layer
struct MlpConcLayout {
  int n_conc, q_idx[PM_MAXL];
  size_t g_off[PM_MAXL], n_logit, lds;
};
static int mlp_concrete_layers(const pmbrl_mlp_call* c, const pmbrl_mlp_concrete* conc, const MlpLayout& L,
                               MlpConcLayout& Q) {
  Q.n_conc = 0;
  Q.n_logit = 0;
  for (int l = 0; l < PM_MAXL; ++l) {
    Q.q_idx[l] = 0;
    Q.g_off[l] = 0;
    if (!conc->u_d[l]) continue;
    if (l >= L.nl - 1) return fail(-2, "mlp concrete: u_d given for a layer that is not a hidden layer");
    if (!conc->logit_d[l]) return fail(-1, "mlp concrete: a layer with u_d needs logit_d");
    if (!(conc->temp[l] > 0.f)) return fail(-2, "mlp concrete: temp must be > 0");
    if (c->net.keep[l] != 1.f) return fail(-2, "mlp concrete: a concrete layer is not divided by p (keep must be 1)");
    Q.q_idx[l] = Q.n_conc++;
    Q.g_off[l] = Q.n_logit;
    Q.n_logit += (size_t)L.dim[l + 1];
  }
  if (!Q.n_conc) return fail(-2, "mlp concrete: no concrete layer (use pmbrl_mlp_backward)");
  return 0;
}
static int mlp_concrete_layout(const pmbrl_mlp_call* c, const pmbrl_mlp_concrete* conc, MlpLayout& L, MlpConcLayout& Q) {
  int rc = mlp_layout(c, L);
  if (rc) return rc;
  if (!conc) return fail(-1, "null argument");
  if ((rc = mlp_concrete_layers(c, conc, L, Q))) return rc;
  Q.lds = pm_mlp_bwdp_lds_floats(L.nl, L.LD, L.act, Q.n_conc) * sizeof(float);
  if (Q.lds > 160 * 1024)
    return fail(-3, "mlp: network too wide / deep for the concrete backward kernel's LDS budget (160 KB)");
  return 0;
}
// a pmbrl_mlp_backward_ln call with layer-norm layers: the concrete layers (conc may be null), the layer-norm layers
// behind their Q buffers, the LDS need of both in N_lds
static int mlp_ln_backward_layout(const pmbrl_mlp_call* c, const pmbrl_mlp_concrete* conc, const pmbrl_mlp_layer_norm* ln,
                                  MlpLayout& L, MlpConcLayout& Q, MlpLnLayout& N, size_t& lds) {
  int rc = mlp_layout(c, L);
  if (rc) return rc;
  memset(&Q, 0, sizeof(Q));
  if (conc && (rc = mlp_concrete_layers(c, conc, L, Q))) return rc;
  if ((rc = mlp_ln_layout(ln, L, Q.n_conc, N))) return rc;
  lds = pm_mlp_bwdp_lds_floats(L.nl, L.LD, L.act, Q.n_conc, N.n_ln) * sizeof(float);
  if (lds > 160 * 1024)
    return fail(-3, "mlp: network too wide / deep for the layer-norm backward kernel's LDS budget (160 KB)");
  return 0;
}
// the layer-norm slabs follow the logit slabs (none: the parameter slabs)
static size_t mlp_ln_slab_offset(const pmbrl_mlp_call* c, const MlpLayout& L, const MlpConcLayout& Q) {
  return (mlp_logit_slab_offset(c, L) + (size_t)mlp_backward_blocks(c, L) * Q.n_logit * sizeof(float) + 255) & ~(size_t)255;
}
// the logit slabs follow the parameter slabs
static size_t mlp_logit_slab_offset(const pmbrl_mlp_call* c, const MlpLayout& L) {
  return (mlp_slab_offset(L) + (size_t)mlp_backward_blocks(c, L) * L.n_params * sizeof(float) + 255) & ~(size_t)255;
}

extern "C" size_t pmbrl_mlp_backward_concrete_workspace_bytes(const pmbrl_mlp_call* c, const pmbrl_mlp_concrete* conc) {
  MlpLayout L;
  MlpConcLayout Q;
  if (mlp_concrete_layout(c, conc, L, Q)) return 0;
  return mlp_logit_slab_offset(c, L) + (size_t)mlp_backward_blocks(c, L) * Q.n_logit * sizeof(float);
}

extern "C" size_t pmbrl_mlp_backward_ln_workspace_bytes(const pmbrl_mlp_call* c, const pmbrl_mlp_concrete* conc,
                                                        const pmbrl_mlp_layer_norm* ln) {
  if (!ln) return conc ? pmbrl_mlp_backward_concrete_workspace_bytes(c, conc) : pmbrl_mlp_backward_workspace_bytes(c);
  MlpLayout L;
  MlpConcLayout Q;
  MlpLnLayout N;
  size_t lds;
  if (mlp_ln_backward_layout(c, conc, ln, L, Q, N, lds)) return 0;
  return mlp_ln_slab_offset(c, L, Q) + (size_t)mlp_backward_blocks(c, L) * N.n_gb * sizeof(float);
}

// pmbrl_mlp_backward (conc == ln == nullptr), pmbrl_mlp_backward_concrete and pmbrl_mlp_backward_ln: one marshalling, the
// kernel's four instances
static int mlp_backward_run(void* stream, const pmbrl_mlp_call* c, void* workspace_d,
                            const float* x_d, const float* params_flat_d,
                            const uint16_t* const* mask_bits_d, const float* z_d,
                            const float* in_shift_d, const float* in_iscale_d,
                            const float* out_scale_d, const float* out_shift_d,
                            const float* sq_scale_d, const float* sq_bias_d,
                            const float* g_sample_d, const float* g_mean_d, const float* g_log_std_d,
                            float* grad_x_d, float* grad_params_d, const pmbrl_mlp_concrete* conc, float* grad_logit_d,
                            const pmbrl_mlp_layer_norm* ln, float* grad_ln_d) {
  MlpLayout L;
  MlpConcLayout Q;
  MlpLnLayout N;
  size_t lds_ln = 0;
  int rc = ln ? mlp_ln_backward_layout(c, conc, ln, L, Q, N, lds_ln)
              : conc ? mlp_concrete_layout(c, conc, L, Q) : mlp_backward_layout(c, L);
  if (rc) return rc;
  if (conc && !grad_logit_d) return fail(-1, "null argument");
  if (!workspace_d || !x_d || !params_flat_d) return fail(-1, "null argument");
  if (!g_sample_d && !g_mean_d && !g_log_std_d) return fail(-1, "mlp backward: no upstream gradient given");
  if ((in_shift_d == nullptr) != (in_iscale_d == nullptr) || (out_scale_d == nullptr) != (out_shift_d == nullptr) ||
      (sq_scale_d == nullptr) != (sq_bias_d == nullptr))
    return fail(-1, "mlp: shift/scale pointers come in pairs");
  if (!grad_x_d && !grad_params_d && !conc && !grad_ln_d) return 0;
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace_d);
  PackArgs PK;
  PK.wflag = nullptr;
  PK.gen = 0;
  PK.n = 0;
  PK.status = nullptr;
  MlpBwdPArgs P;
  memset(&P, 0, sizeof(P));
  MlpArgs& A = P.b.f;
  A.B = c->B; A.nl = L.nl; A.LD = L.LD; A.n_out = L.dim[L.nl] / 2;
  for (int i = 0; i <= L.nl; ++i) { A.dim[i] = L.dim[i]; A.nt[i] = L.nt[i]; }
  for (int l = 0; l < L.nl; ++l) {
    float* wf = reinterpret_cast<float*>(ws + L.wf[l]);
    float* wb = reinterpret_cast<float*>(ws + L.wb[l]);
    float* bs = reinterpret_cast<float*>(ws + L.bias[l]);
    PK.job[PK.n++] = PackJob{params_flat_d + L.w_off[l], wf, L.dim[l + 1], L.dim[l], 0, 1, 0, 0, 0};
    PK.job[PK.n++] = PackJob{params_flat_d + L.w_off[l], wb, L.dim[l + 1], L.dim[l], 1, 1, 0, 0, 0};
    PK.job[PK.n++] = PackJob{params_flat_d + L.b_off[l], bs, L.dim[l + 1], L.dim[l], 0, 1, 1, 0, 0};
    A.wf[l] = wf; P.b.wb[l] = wb; A.bias[l] = bs;
    A.mask[l] = (l < L.nl - 1 && mask_bits_d) ? mask_bits_d[l] : nullptr;
    A.keep[l] = l < L.nl - 1 ? c->net.keep[l] : 1.f;
    P.w_off[l] = L.w_off[l];
    P.b_off[l] = L.b_off[l];
  }
  A.x = x_d; A.z = z_d; A.in_shift = in_shift_d; A.in_iscale = in_iscale_d;
  A.out_scale = out_scale_d; A.out_shift = out_shift_d; A.sq_scale = sq_scale_d; A.sq_bias = sq_bias_d;
  A.mls = c->max_log_std;
  A.act = L.act;
  P.b.g_sample = g_sample_d; P.b.g_mean = g_mean_d; P.b.g_log_std = g_log_std_d; P.b.grad_x = grad_x_d;
  const int n_blocks = mlp_backward_blocks(c, L);
  P.n_params = L.n_params;
  P.slab = grad_params_d ? reinterpret_cast<float*>(ws + mlp_slab_offset(L)) : nullptr;
  pm_pack_all_launch(PK, s);
  if (ln) {
    MlpBwdLArgs La;
    memset(&La, 0, sizeof(La));
    La.p = P;
    if (conc) {
      for (int l = 0; l < L.nl - 1; ++l) {
        La.c.u[l] = conc->u_d[l];
        La.c.logit[l] = conc->logit_d[l];
        La.c.temp[l] = conc->temp[l];
        La.c.q_idx[l] = Q.q_idx[l];
        La.c.g_off[l] = Q.g_off[l];
      }
      La.c.slab = reinterpret_cast<float*>(ws + mlp_logit_slab_offset(c, L));
      La.c.n_logit = Q.n_logit;
    }
    mlp_ln_args(ln, L, N, La.ln);
    La.ln.slab = grad_ln_d ? reinterpret_cast<float*>(ws + mlp_ln_slab_offset(c, L, Q)) : nullptr;
    if ((rc = pm_mlp_ln_launch_bwdp(s, n_blocks, lds_ln, La, conc != nullptr))) return rc;
    if (conc) {
      hipLaunchKernelGGL(pm_mlp_bwd_reduce_kernel, dim3((unsigned)((Q.n_logit + 255) / 256)), dim3(256), 0, s, La.c.slab,
                         n_blocks, Q.n_logit, grad_logit_d);
      HIPCHK(hipGetLastError());
    }
    if (grad_ln_d) {
      hipLaunchKernelGGL(pm_mlp_bwd_reduce_kernel, dim3((unsigned)((N.n_gb + 255) / 256)), dim3(256), 0, s, La.ln.slab,
                         n_blocks, N.n_gb, grad_ln_d);
      HIPCHK(hipGetLastError());
    }
  } else if (conc) {
    MlpBwdCArgs Cc;
    memset(&Cc, 0, sizeof(Cc));
    Cc.p = P;
    for (int l = 0; l < L.nl - 1; ++l) {
      Cc.c.u[l] = conc->u_d[l];
      Cc.c.logit[l] = conc->logit_d[l];
      Cc.c.temp[l] = conc->temp[l];
      Cc.c.q_idx[l] = Q.q_idx[l];
      Cc.c.g_off[l] = Q.g_off[l];
    }
    Cc.c.slab = reinterpret_cast<float*>(ws + mlp_logit_slab_offset(c, L));
    Cc.c.n_logit = Q.n_logit;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_mlp_bwdp_kernel<true, false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)Q.lds));
    hipLaunchKernelGGL((pm_mlp_bwdp_kernel<true, false>), dim3(n_blocks), dim3(PM_NT), Q.lds, s, Cc);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(pm_mlp_bwd_reduce_kernel, dim3((unsigned)((Q.n_logit + 255) / 256)), dim3(256), 0, s, Cc.c.slab,
                       n_blocks, Q.n_logit, grad_logit_d);
    HIPCHK(hipGetLastError());
  } else {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_mlp_bwdp_kernel<false, false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds_bwdp));
    hipLaunchKernelGGL((pm_mlp_bwdp_kernel<false, false>), dim3(n_blocks), dim3(PM_NT), L.lds_bwdp, s, P);
    HIPCHK(hipGetLastError());
  }
  if (grad_params_d) {
    hipLaunchKernelGGL(pm_mlp_bwd_reduce_kernel, dim3((unsigned)((L.n_params + 255) / 256)), dim3(256), 0, s, P.slab,
                       n_blocks, L.n_params, grad_params_d);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

extern "C" int pmbrl_mlp_backward(void* stream, const pmbrl_mlp_call* c, void* workspace_d,
                                  const float* x_d, const float* params_flat_d,
                                  const uint16_t* const* mask_bits_d, const float* z_d,
                                  const float* in_shift_d, const float* in_iscale_d,
                                  const float* out_scale_d, const float* out_shift_d,
                                  const float* sq_scale_d, const float* sq_bias_d,
                                  const float* g_sample_d, const float* g_mean_d, const float* g_log_std_d,
                                  float* grad_x_d, float* grad_params_d) {
  return mlp_backward_run(stream, c, workspace_d, x_d, params_flat_d, mask_bits_d, z_d, in_shift_d, in_iscale_d, out_scale_d,
                          out_shift_d, sq_scale_d, sq_bias_d, g_sample_d, g_mean_d, g_log_std_d, grad_x_d, grad_params_d,
                          nullptr, nullptr, nullptr, nullptr);
}

extern "C" int pmbrl_mlp_backward_concrete(void* stream, const pmbrl_mlp_call* c, void* workspace_d,
                                           const float* x_d, const float* params_flat_d,
                                           const uint16_t* const* mask_bits_d, const float* z_d,
                                           const float* in_shift_d, const float* in_iscale_d,
                                           const float* out_scale_d, const float* out_shift_d,
                                           const float* sq_scale_d, const float* sq_bias_d,
                                           const float* g_sample_d, const float* g_mean_d, const float* g_log_std_d,
                                           float* grad_x_d, float* grad_params_d, const pmbrl_mlp_concrete* conc,
                                           float* grad_logit_d) {
  if (!conc) return fail(-1, "null argument");
  return mlp_backward_run(stream, c, workspace_d, x_d, params_flat_d, mask_bits_d, z_d, in_shift_d, in_iscale_d, out_scale_d,
                          out_shift_d, sq_scale_d, sq_bias_d, g_sample_d, g_mean_d, g_log_std_d, grad_x_d, grad_params_d,
                          conc, grad_logit_d, nullptr, nullptr);
}

extern "C" int pmbrl_mlp_backward_ln(void* stream, const pmbrl_mlp_call* c, void* workspace_d,
                                     const float* x_d, const float* params_flat_d,
                                     const uint16_t* const* mask_bits_d, const float* z_d,
                                     const float* in_shift_d, const float* in_iscale_d,
                                     const float* out_scale_d, const float* out_shift_d,
                                     const float* sq_scale_d, const float* sq_bias_d,
                                     const float* g_sample_d, const float* g_mean_d, const float* g_log_std_d,
                                     float* grad_x_d, float* grad_params_d, const pmbrl_mlp_concrete* conc,
                                     float* grad_logit_d, const pmbrl_mlp_layer_norm* ln, float* grad_ln_d) {
  return mlp_backward_run(stream, c, workspace_d, x_d, params_flat_d, mask_bits_d, z_d, in_shift_d, in_iscale_d, out_scale_d,
                          out_shift_d, sq_scale_d, sq_bias_d, g_sample_d, g_mean_d, g_log_std_d, grad_x_d, grad_params_d,
                          conc, grad_logit_d, ln, grad_ln_d);
}
