// BNN training step (pmbrl_bnn.h): the plan, loss and gradient of one minibatch, whole training iterations.  The weight
// packer, the dW block kernel and its reduction are other objects': reached through their launchers (pmbrl_host.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pmbrl_host.h"
#include "pmbrl_mm.h"
#include "pmbrl_rollout.h"
#include "pmbrl_bnn.h"

// the instances a plan launches
struct BnnKernels {
  void (*fwd_bwd)(const BnnArgs);
  void (*finish)(const BnnFinishArgs);
  void (*tail)(const BnnTailArgs);
  void (*tail_rule)(const BnnTailRuleArgs);   // with an optimiser rule attached (pmbrl_bnn_plan_set_optimizer)
};
// ... chosen HERE and nowhere else: a plan without a Bernoulli layer launches the instances it always did
static BnnKernels bnn_kernels(int act, int any_bern) {
  if (any_bern) return {act ? pm_bnn_fwd_bwd<true, true> : pm_bnn_fwd_bwd<false, true>, pm_bnn_finish<true>, pm_bnn_tail<true>,
            pm_bnn_tail<true, BnnTailRuleArgs>};
  return {act ? pm_bnn_fwd_bwd<true> : pm_bnn_fwd_bwd<false>, pm_bnn_finish<false>, pm_bnn_tail<false>,
          pm_bnn_tail<false, BnnTailRuleArgs>};
}

struct pmbrl_bnn_plan {
  pmbrl_bnn_config cfg;
  int device, nl, LD, nwg, sum_h, n_params;
  int acts;       // PMBRL_ACT_* per hidden layer (pm_act_layers of cfg.act); 0: every layer is ReLU
  int dim[PM_MAXL + 1], nt[PM_MAXL + 1];
  int w_off[PM_MAXL], b_off[PM_MAXL], lp_poff[PM_MAXL], lp_off[PM_MAXL], has_drop[PM_MAXL];
  size_t off_wf[PM_MAXL], off_wb[PM_MAXL], off_bias[PM_MAXL], off_actT[PM_MAXL], off_gT[PM_MAXL];
  size_t off_part_lp, off_part_loss, off_part, off_reg_part, ws_bytes, lds;
  int part_stride, dw_wave_first[PM_DW_NW + 1];
  DwBlock* dw_blocks_d;
  // fixed-rate Bernoulli layers (has_drop[l] == 2): noise_off / noise_h count the dropout layers of EITHER kind (the
  // u / bvar blocks), lp_off / sum_h the concrete ones (the logit gradients); keep_d[l]: the units' keep probabilities
  int noise_off[PM_MAXL], noise_h, any_bern;
  float* keep_d[PM_MAXL];
  float* keep_all_d;
  BnnKernels kern;
  // What the kernels' argument records hold of the plan alone (bnn_plan_records; as DwPlan::args).  A call starts
  // from a COPY -- the two calls alternate on one plan -- and adds its workspace and parameter pointers (bnn_bind) and
  // what is the call's own; everything else in them stays zero.
  BnnArgs args;
  BnnFinishArgs fin;
  BnnTailArgs tail;
  DwArgs dw;
  int n_finish;   // workgroups of pm_bnn_finish
  // PMBRL_BNN_FORM_RESIDENT or _SPILL: which kernel the forward + backward launch is (bnn_fwd_bwd_launch); a spill plan's
  // lds is pm_bnn_spill_lds_floats', its workspace holds the stashes of BnnSpillArgs::hq (off_spill)
  int form;
  size_t off_spill;
  int units;      // workgroups of pm_bnn_tail (more than 512: pmbrl_bnn_train_steps refuses)
  // optimiser rule (pmbrl_bnn_plan_set_optimizer): the groups of the layers' tensors, resolved when it was attached
  int has_rule;
  pmbrl_opt_rule rule;
  int grp_w[PM_MAXL], grp_b[PM_MAXL], grp_lp[PM_MAXL];
};

static void bnn_plan_records(pmbrl_bnn_plan* p) {
  const pmbrl_bnn_config& c = p->cfg;
  BnnArgs& A = p->args;
  BnnFinishArgs& F = p->fin;
  BnnTailArgs& T = p->tail;
  DwArgs& W = p->dw;
  memset(&A, 0, sizeof(A));
  memset(&F, 0, sizeof(F));
  memset(&T, 0, sizeof(T));
  memset(&W, 0, sizeof(W));
  A.M = c.M; A.nl = p->nl; A.LD = p->LD; A.n_out = p->dim[p->nl] / 2; A.nwg = p->nwg;
  if (c.loss_kind == 2) {
    A.gmm_n = c.n_components;
    A.n_out = ((p->dim[p->nl] - 1) / A.gmm_n - 1) / 2;
  }
  A.n_in = p->dim[0]; A.sum_h = p->sum_h;
  A.act = p->acts;
  A.mls = c.max_log_std;
  A.mse = c.loss_kind == 1;
  A.inv_M = F.inv_M = T.inv_M = 1.f / (float)c.M;
  F.nl = T.nl = p->nl; F.nwg = p->nwg; F.sum_h = T.sum_h = p->sum_h; F.N = T.N = c.N;
  T.n_chunks = T.n_part_loss = p->nwg;
  T.reg_weight = c.reg_weight;      // (pm_bnn_finish's is the call's: terms)
  // dW / db of every layer: the policy-gradient GEMM over the same stash layout (one 16-row chunk per split)
  W.nl = p->nl; W.nsplit = p->nwg; W.n_chunks = p->nwg; W.chunks_per_split = 1;
  W.RT = 1; W.Rw = 16; W.n_params = p->n_params; W.part_stride = p->part_stride;
  pm_dw_bind_blocks(W, p->dw_blocks_d, p->dw_wave_first);
  for (int i = 0; i <= p->nl; ++i) {
    A.dim[i] = F.dim[i] = T.dim[i] = W.dim[i] = p->dim[i];
    A.nt[i] = T.nt[i] = W.nt[i] = p->nt[i];
  }
  p->units = 0;
  p->n_finish = 0;
  for (int l = 0; l < p->nl; ++l) {
    F.w_off[l] = T.w_off[l] = W.w_off[l] = p->w_off[l];
    F.b_off[l] = T.b_off[l] = W.b_off[l] = p->b_off[l];
    F.lp_poff[l] = T.lp_poff[l] = p->lp_poff[l];
    A.lp_off[l] = F.lp_off[l] = T.lp_off[l] = p->lp_off[l];
    F.has_drop[l] = T.has_drop[l] = p->has_drop[l];
    F.keep[l] = T.keep[l] = p->keep_d[l];
    F.reg_scale[l] = T.reg_scale[l] = c.reg_scale[l];
    F.drop_reg[l] = T.drop_reg[l] = c.drop_reg[l];
    if (p->has_drop[l] == 1) A.inv_temp[l] = 1.f / c.temperature[l];
    else if (p->has_drop[l] == 2) A.keep[l] = p->keep_d[l];
    T.unit0[l] = p->units;
    p->units += p->nt[l];
    if (l < p->nl - 1 && p->has_drop[l]) p->n_finish += (p->dim[l + 1] + PM_BNN_CG - 1) / PM_BNN_CG;
  }
  T.unit0[p->nl] = p->units;
  if (p->n_finish < 1) p->n_finish = 1;
}

// A call's pointers into its workspace and its parameter vector: into A, a copy of the plan's record (the other records
// take theirs from it), and the packer's jobs
static PackArgs bnn_bind(const pmbrl_bnn_plan* p, char* ws, const float* params_flat_d, BnnArgs& A) {
  PackArgs PK;
  PK.wflag = nullptr;
  PK.gen = 0;
  PK.n = 0;
  PK.status = nullptr;
  for (int l = 0; l < p->nl; ++l) {
    float* wf = reinterpret_cast<float*>(ws + p->off_wf[l]);
    float* wb = reinterpret_cast<float*>(ws + p->off_wb[l]);
    float* bs = reinterpret_cast<float*>(ws + p->off_bias[l]);
    PK.job[PK.n++] = PackJob{params_flat_d + p->w_off[l], wf, p->dim[l + 1], p->dim[l], 0, 1, 0, 0, 0};
    PK.job[PK.n++] = PackJob{params_flat_d + p->w_off[l], wb, p->dim[l + 1], p->dim[l], 1, 1, 0, 0, 0};
    PK.job[PK.n++] = PackJob{params_flat_d + p->b_off[l], bs, p->dim[l + 1], p->dim[l], 0, 1, 1, 0, 0};
    A.wf[l] = wf; A.wb[l] = wb; A.bias[l] = bs;
    A.actT[l] = reinterpret_cast<float*>(ws + p->off_actT[l]);
    A.gT[l] = reinterpret_cast<float*>(ws + p->off_gT[l]);
    if (p->has_drop[l] == 1) A.logit_p[l] = params_flat_d + p->lp_poff[l];
  }
  A.part_lp = reinterpret_cast<float*>(ws + p->off_part_lp);
  A.part_loss = reinterpret_cast<float*>(ws + p->off_part_loss);
  return PK;
}

// the forward + backward launch of a call, in the plan's form
static void bnn_fwd_bwd_launch(const pmbrl_bnn_plan* p, const BnnArgs& A, char* ws, hipStream_t s) {
  if (p->form == PMBRL_BNN_FORM_SPILL) {
    BnnSpillArgs S;
    static_cast<BnnArgs&>(S) = A;
    S.hq = reinterpret_cast<float*>(ws + p->off_spill);
    pm_bnn_spill_launch(S, p->acts != 0, p->any_bern, p->lds, s);
  } else {
    hipLaunchKernelGGL(p->kern.fwd_bwd, dim3(p->nwg), dim3(PM_NT), p->lds, s, A);
  }
}

extern "C" int pmbrl_bnn_plan_create_form(const pmbrl_bnn_config* cfg, int device, int32_t form, pmbrl_bnn_plan** out) {
  if (!cfg || !out) return fail(-1, "null argument");
  if (form != PMBRL_BNN_FORM_RESIDENT && form != PMBRL_BNN_FORM_SPILL && form != PMBRL_BNN_FORM_AUTO)
    return fail(-2, "bnn: unknown kernel form (PMBRL_BNN_FORM_RESIDENT, _SPILL and _AUTO are offered)");
  const pmbrl_mlp& m = cfg->net;
  if (m.n_layers < 2 || m.n_layers > PM_MAXL) return fail(-2, "bnn: 2..8 layers");
  if (cfg->M < 1 || cfg->N < 1) return fail(-2, "bnn: M, N must be >= 1");
  if (cfg->loss_kind == 2) {
    const int n = cfg->n_components;
    if (n < 2 || n > PMBRL_MAX_COMP) return fail(-2, "bnn: mixture loss needs 2..PMBRL_MAX_COMP components");
    if ((m.dims[m.n_layers] - 1) % n || ((m.dims[m.n_layers] - 1) / n - 1) % 2 || (m.dims[m.n_layers] - 1) / n < 3)
      return fail(-2, "bnn: mixture head must be (2 n_out + 1) n_components + 1 wide");
  } else if (m.dims[m.n_layers] % 2) return fail(-2, "bnn: the output layer must be 2 x n_out wide");
  pmbrl_bnn_plan* p = new pmbrl_bnn_plan();
  p->cfg = *cfg;
  p->device = device;
  p->nl = m.n_layers;
  int maxnt = 1, po = 0;
  p->sum_h = 0;
  p->noise_h = 0;
  p->any_bern = 0;
  for (int l = 0; l < p->nl - 1; ++l) {
    if (cfg->drop_kind[l] != PMBRL_DROP_BY_TEMPERATURE && cfg->drop_kind[l] != PMBRL_DROP_BERNOULLI) {
      delete p;
      return fail(-2, "bnn: unknown dropout kind (0: by temperature, PMBRL_DROP_BERNOULLI are offered)");
    }
    if (cfg->drop_kind[l] == PMBRL_DROP_BERNOULLI && !(cfg->bern_keep[l] > 0.f && cfg->bern_keep[l] <= 1.f)) {
      delete p;
      return fail(-2, "bnn: the keep probability of a Bernoulli layer must lie in (0, 1]");
    }
  }
  for (int i = 0; i <= p->nl; ++i) {
    if (m.dims[i] < 1 || m.dims[i] > 16 * 64) { delete p; return fail(-2, "bnn: layer width out of range"); }
    p->dim[i] = m.dims[i];
    p->nt[i] = (m.dims[i] + 15) / 16;
    maxnt = std::max(maxnt, p->nt[i]);
  }
  for (int l = 0; l < p->nl; ++l) {
    p->w_off[l] = po; po += p->dim[l + 1] * p->dim[l];
    p->b_off[l] = po; po += p->dim[l + 1];
    p->has_drop[l] = 0;
    if (l < p->nl - 1) {
      if (cfg->drop_kind[l] == PMBRL_DROP_BERNOULLI) p->has_drop[l] = 2;
      else if (cfg->temperature[l] > 0.f) p->has_drop[l] = 1;
    }
    p->lp_poff[l] = po;
    p->lp_off[l] = p->sum_h;
    p->noise_off[l] = p->noise_h;
    if (p->has_drop[l] == 1) { po += p->dim[l + 1]; p->sum_h += p->dim[l + 1]; }
    if (p->has_drop[l]) p->noise_h += p->dim[l + 1];
    if (p->has_drop[l] == 2) p->any_bern = 1;
  }
  p->n_params = po;
  p->LD = maxnt * 16 + 8;
  p->nwg = (cfg->M + 15) / 16;
  if (const char* why = pm_act_refusal(cfg->act, p->nl - 1)) {
    delete p;
    return fail(-2, std::string("bnn: ") + why);
  }
  p->acts = pm_act_layers(cfg->act, p->nl - 1);
  p->lds = pm_bnn_lds_floats(p->nl, p->LD, p->acts) * sizeof(float);
  p->form = PMBRL_BNN_FORM_RESIDENT;
  if (form == PMBRL_BNN_FORM_SPILL || (form == PMBRL_BNN_FORM_AUTO && p->lds > 160 * 1024)) {
    p->form = PMBRL_BNN_FORM_SPILL;
    p->lds = pm_bnn_spill_lds_floats(p->LD) * sizeof(float);
    if (p->lds + PM_BNN_LDS_STATIC > 160 * 1024) {
      delete p;
      return fail(-3, "bnn: network too wide for the spill form's LDS budget (three [16][LD] buffers: at most 688 units a layer)");
    }
  } else if (p->lds > 160 * 1024) { delete p; return fail(-3, "bnn: network too wide / deep for the fused training step's LDS budget"); }
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  for (int l = 0; l < p->nl; ++l) {
    p->off_wf[l] = take((size_t)p->nt[l + 1] * p->nt[l] * 256 * sizeof(float));
    p->off_wb[l] = take((size_t)p->nt[l + 1] * p->nt[l] * 256 * sizeof(float));
    p->off_bias[l] = take((size_t)p->nt[l + 1] * 16 * sizeof(float));
    p->off_actT[l] = take((size_t)p->nwg * p->nt[l] * 16 * 16 * sizeof(float));
    p->off_gT[l] = take((size_t)p->nwg * p->nt[l + 1] * 16 * 16 * sizeof(float));
  }
  p->part_stride = (p->n_params + 3) / 4 * 4;
  p->off_part_lp = take((size_t)p->nwg * std::max(p->sum_h, 1) * sizeof(float));
  p->off_part_loss = take((size_t)p->nwg * sizeof(float));
  p->off_part = take((size_t)p->nwg * p->part_stride * sizeof(float));
  // (a spill plan's stashes in front of the scratch, which stays the workspace's last 4 KB)
  if (p->form == PMBRL_BNN_FORM_SPILL) p->off_spill = take(pm_bnn_spill_stash_floats(p->nwg, p->nl, p->LD) * sizeof(float));
  p->off_reg_part = take(1024 * sizeof(float));
  p->ws_bytes = off;
  HIPCHK(hipSetDevice(device));
  std::vector<DwBlock> blocks;
  build_dw_blocks(p->nl, p->nt, blocks, p->dw_wave_first);
  HIPCHK(pm_dw_upload_blocks(blocks, &p->dw_blocks_d));
  if (p->any_bern) {
    // the Bernoulli layers' keep probabilities, one per unit (a scalar rate repeated; the padding of the last tile keeps 1)
    std::vector<float> keep;
    size_t koff[PM_MAXL] = {0};
    for (int l = 0; l < p->nl - 1; ++l)
      if (p->has_drop[l] == 2) {
        koff[l] = keep.size();
        keep.resize(keep.size() + (size_t)p->nt[l + 1] * 16, 1.f);
        for (int j = 0; j < p->dim[l + 1]; ++j) keep[koff[l] + j] = cfg->bern_keep[l];
      }
    HIPCHK(hipMalloc(&p->keep_all_d, keep.size() * sizeof(float)));
    HIPCHK(hipMemcpy(p->keep_all_d, keep.data(), keep.size() * sizeof(float), hipMemcpyHostToDevice));
    for (int l = 0; l < p->nl - 1; ++l)
      if (p->has_drop[l] == 2) p->keep_d[l] = p->keep_all_d + koff[l];
  }
  p->kern = bnn_kernels(p->acts, p->any_bern);
  if (p->form == PMBRL_BNN_FORM_SPILL) HIPCHK(pm_bnn_spill_prepare(p->acts != 0, p->any_bern));
  else HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(p->kern.fwd_bwd), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)p->lds));
  bnn_plan_records(p);
  *out = p;
  return 0;
}

extern "C" int pmbrl_bnn_plan_create(const pmbrl_bnn_config* cfg, int device, pmbrl_bnn_plan** out) {
  return pmbrl_bnn_plan_create_form(cfg, device, PMBRL_BNN_FORM_RESIDENT, out);
}
extern "C" int32_t pmbrl_bnn_plan_form(const pmbrl_bnn_plan* p) { return p ? p->form : -1; }

extern "C" void pmbrl_bnn_plan_destroy(pmbrl_bnn_plan* p) {
  if (!p) return;
  if (p->dw_blocks_d) (void)hipFree(p->dw_blocks_d);
  if (p->keep_all_d) (void)hipFree(p->keep_all_d);
  delete p;
}

extern "C" int pmbrl_bnn_plan_set_unit_keep(pmbrl_bnn_plan* p, int32_t layer, const float* keep_h, int32_t n) {
  if (!p || !keep_h) return fail(-1, "null argument");
  if (layer < 0 || layer >= p->nl - 1 || p->has_drop[layer] != 2)
    return fail(-2, "pmbrl_bnn_plan_set_unit_keep: not a Bernoulli layer of this plan");
  if (n != p->dim[layer + 1]) return fail(-2, "pmbrl_bnn_plan_set_unit_keep: n must be the layer's width");
  for (int j = 0; j < n; ++j)
    if (!(keep_h[j] > 0.f && keep_h[j] <= 1.f))
      return fail(-2, "pmbrl_bnn_plan_set_unit_keep: keep probabilities must lie in (0, 1]");
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(hipDeviceSynchronize());      // (a step of this plan may still be reading the old values)
  HIPCHK(hipMemcpy(p->keep_d[layer], keep_h, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}
// the group of the tensor [off, off + len) of the flat vector, -1 if it does not lie in one segment
static int bnn_rule_group(const pmbrl_opt_rule& r, int64_t off, int64_t len) {
  int64_t lo = 0;
  for (int q = 0; q < r.n_segments; ++q) {
    if (off >= lo && off < r.seg_end[q]) return off + len <= r.seg_end[q] ? r.seg_group[q] : -1;
    lo = r.seg_end[q];
  }
  return -1;
}
extern "C" int pmbrl_bnn_plan_set_optimizer(pmbrl_bnn_plan* p, const pmbrl_opt_rule* rule) {
  if (!p) return fail(-1, "null plan");
  if (!rule) { p->has_rule = 0; return 0; }
  if (int rc = pmbrl_opt_rule_check(rule, (int64_t)p->n_params)) return rc;
  int gw[PM_MAXL] = {0}, gb[PM_MAXL] = {0}, glp[PM_MAXL] = {0};
  for (int l = 0; l < p->nl; ++l) {
    gw[l] = bnn_rule_group(*rule, p->w_off[l], (int64_t)p->dim[l + 1] * p->dim[l]);
    gb[l] = bnn_rule_group(*rule, p->b_off[l], p->dim[l + 1]);
    glp[l] = p->has_drop[l] == 1 ? bnn_rule_group(*rule, p->lp_poff[l], p->dim[l + 1]) : 0;
    if (gw[l] < 0 || gb[l] < 0 || glp[l] < 0)
      return fail(-2, "pmbrl_bnn_plan_set_optimizer: a weight, bias or logit tensor of the network lies in more than one segment");
  }
  p->rule = *rule;
  for (int l = 0; l < p->nl; ++l) { p->grp_w[l] = gw[l]; p->grp_b[l] = gb[l]; p->grp_lp[l] = glp[l]; }
  p->has_rule = 1;
  return 0;
}
static BnnOptRec bnn_opt_rec(const pmbrl_opt_group& G) {
  BnnOptRec r;
  const OptGroupConsts c = pm_opt_group_consts(G);
  r.lr = (float)G.lr; r.b1 = (float)G.beta1; r.b2 = (float)G.beta2; r.eps = (float)G.eps;
  r.wd = c.wd; r.decay = c.decay; r.sgn = c.sgn; r.ams = c.ams;
  r.ln_b1 = c.ln_b1; r.ln_b2 = c.ln_b2;
  return r;
}
extern "C" size_t pmbrl_bnn_plan_workspace_bytes(const pmbrl_bnn_plan* p) { return p ? p->ws_bytes : 0; }
extern "C" int64_t pmbrl_bnn_plan_n_params(const pmbrl_bnn_plan* p) { return p ? p->n_params : 0; }

extern "C" int pmbrl_bnn_loss_grad_ex(pmbrl_bnn_plan* p, void* stream, void* workspace_d, const float* Xn_d,
                                      const float* Yn_d, const int32_t* idx_d, const float* params_flat_d,
                                      const float* u_d, const float* bvar_d, float* grad_flat_d,
                                      float* loss_out_d, const float* row_weight_d, float* row_logprob_d,
                                      int32_t terms) {
  if (!p || !workspace_d || !Xn_d || !Yn_d || !idx_d || !params_flat_d || !grad_flat_d || !loss_out_d)
    return fail(-1, "null argument");
  if (!(terms & 3)) return fail(-1, "bnn: terms must select the likelihood (1), the regulariser (2) or both");
  const bool lik = (terms & 1) != 0, regt = (terms & 2) != 0;
  if (lik && ((p->sum_h > 0 && !u_d) || (p->noise_h > 0 && !bvar_d))) return fail(-1, "bnn: dropout layers need u and bvar");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(p->device));
  char* ws = static_cast<char*>(workspace_d);
  BnnArgs A = p->args;
  const PackArgs PK = bnn_bind(p, ws, params_flat_d, A);
  for (int l = 0; l < p->nl; ++l) {
    if (p->has_drop[l] == 1) A.u[l] = u_d + (size_t)p->cfg.M * p->noise_off[l];
    if (p->has_drop[l]) A.bvar[l] = bvar_d + (size_t)p->cfg.M * p->noise_off[l];
  }
  A.X = Xn_d; A.Y = Yn_d; A.idx = idx_d;
  A.row_w = row_weight_d; A.row_lp = row_logprob_d;
  if (!lik) {
    HIPCHK(hipMemsetAsync(grad_flat_d, 0, (size_t)p->n_params * sizeof(float), s));
  } else {
    pm_pack_all_launch(PK, s);
    bnn_fwd_bwd_launch(p, A, ws, s);
    DwArgs W = p->dw;
    for (int l = 0; l < p->nl; ++l) { W.actT[l] = A.actT[l]; W.gT[l] = A.gT[l]; }
    W.part = reinterpret_cast<float*>(ws + p->off_part);
    pm_dw_blocks_launch(W, s);
    pm_dw_reduce_launch(s, W.part, p->nwg, p->n_params, p->part_stride, grad_flat_d, (const int*)nullptr, 0, 1);
  }
  BnnFinishArgs Fa = p->fin;
  Fa.reg_weight = regt ? p->cfg.reg_weight : 0.f;
  Fa.reg_only = lik ? 0 : 1;
  Fa.params = params_flat_d; Fa.grad = grad_flat_d; Fa.part_lp = A.part_lp; Fa.part_loss = A.part_loss;
  Fa.loss_out = loss_out_d; Fa.reg_part = reinterpret_cast<float*>(ws + p->off_reg_part);
  hipLaunchKernelGGL(p->kern.finish, dim3(p->n_finish), dim3(256), 0, s, Fa);
  hipLaunchKernelGGL(pm_bnn_loss, dim3(1), dim3(64), 0, s, Fa, p->n_finish);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int pmbrl_bnn_loss_grad(pmbrl_bnn_plan* p, void* stream, void* workspace_d, const float* Xn_d,
                                   const float* Yn_d, const int32_t* idx_d, const float* params_flat_d,
                                   const float* u_d, const float* bvar_d, float* grad_flat_d,
                                   float* loss_out_d) {
  return pmbrl_bnn_loss_grad_ex(p, stream, workspace_d, Xn_d, Yn_d, idx_d, params_flat_d, u_d, bvar_d,
                                grad_flat_d, loss_out_d, nullptr, nullptr, 3);
}

// Whole training iterations of utils/train_regressor.py:113-131 (likelihood + regulariser, Adam, no clipping) in TWO
// launches each: pm_bnn_fwd_bwd, pm_bnn_tail (pmbrl_bnn.h).  n_steps iterations are queued by ONE call: minibatch i takes
// rows idx_all_d[i * M ..]; the dropout noise comes from the in-kernel generator (seed, first_step + i) unless recorded
// draws are handed in (u_d / bvar_d: [n_steps][M * sum_h]).  The weights' fragments are packed once at the start of the
// call (the parameters may have changed outside) and kept current by the tail of every iteration.
extern "C" int pmbrl_bnn_train_steps(pmbrl_bnn_plan* p, void* stream, void* workspace_d, const float* Xn_d, const float* Yn_d,
                                     const int32_t* idx_all_d, int32_t n_steps, float* params_flat_d, float* exp_avg_d,
                                     float* exp_avg_sq_d, int64_t* step_d, double lr, double beta1, double beta2, double eps,
                                     uint64_t seed, uint64_t first_step, const float* u_d, const float* bvar_d,
                                     float* loss_out_d, float* loss_hist_d) {
  if (!p || !workspace_d || !Xn_d || !Yn_d || !idx_all_d || !params_flat_d || !exp_avg_d || !exp_avg_sq_d || !step_d ||
      !loss_out_d || n_steps < 1)
    return fail(-1, "bad argument");
  if (p->cfg.loss_kind != 0) return fail(-3, "pmbrl_bnn_train_steps: the diagonal-Gaussian likelihood only (use pmbrl_bnn_loss_grad_ex)");
  if ((u_d == nullptr) != (bvar_d == nullptr)) return fail(-1, "bnn: u and bvar come together");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(p->device));
  char* ws = static_cast<char*>(workspace_d);
  if (p->units > 512) return fail(-3, "pmbrl_bnn_train_steps: network too wide for the fused tail");
  BnnArgs A = p->args;
  const PackArgs PK = bnn_bind(p, ws, params_flat_d, A);
  BnnTailArgs T = p->tail;
  for (int l = 0; l < p->nl; ++l) {
    // (the tail keeps the fragments current: the same buffers, written)
    T.wf[l] = const_cast<float*>(A.wf[l]); T.wb[l] = const_cast<float*>(A.wb[l]); T.bias[l] = const_cast<float*>(A.bias[l]);
    T.actT[l] = A.actT[l]; T.gT[l] = A.gT[l];
  }
  A.X = Xn_d; A.Y = Yn_d;
  T.part_lp = A.part_lp; T.part_loss = A.part_loss;
  T.params = params_flat_d; T.m = exp_avg_d; T.v = exp_avg_sq_d;
  T.reg_part = reinterpret_cast<float*>(ws + p->off_reg_part);
  T.counter = reinterpret_cast<unsigned*>(ws + p->off_reg_part) + 1000;
  T.step = reinterpret_cast<long long*>(step_d);
  T.lr = (float)lr; T.b1 = (float)beta1; T.b2 = (float)beta2; T.eps = (float)eps;
  T.ln_b1 = log(beta1); T.ln_b2 = log(beta2);
  A.rng = u_d ? 0 : 1;
  A.prof = getenv("PMBRL_BNN_PROF") ? reinterpret_cast<long long*>(ws + p->off_reg_part) + 256 : nullptr;      // (debugging: stamps at floats 512.. of the scratch)
  A.rng_k0 = (unsigned)seed; A.rng_k1 = (unsigned)(seed >> 32);
  // a rule attached to the plan: its instance of the tail, the hyper-parameters from the rule (lr .. eps above are ignored)
  BnnTailRuleArgs TR;
  if (p->has_rule) {
    memset(&TR, 0, sizeof(TR));
    bool ams = false;
    for (int l = 0; l < p->nl; ++l) {
      TR.w[l] = bnn_opt_rec(p->rule.group[p->grp_w[l]]);
      TR.b[l] = bnn_opt_rec(p->rule.group[p->grp_b[l]]);
      TR.lp[l] = bnn_opt_rec(p->rule.group[p->grp_lp[l]]);
    }
    for (int k = 0; k < p->rule.n_groups; ++k) ams = ams || (p->rule.group[k].flags & PMBRL_OPT_AMSGRAD);
    TR.vmax = ams ? p->rule.max_exp_avg_sq_d : exp_avg_sq_d;
  }
  HIPCHK(hipMemsetAsync(T.counter, 0, sizeof(unsigned), s));
  pm_pack_all_launch(PK, s);
  const size_t noise = (size_t)p->cfg.M * p->noise_h;
  for (int i = 0; i < n_steps; ++i) {
    A.idx = idx_all_d + (size_t)i * p->cfg.M;
    A.rng_step = (unsigned)(first_step + (uint64_t)i);
    for (int l = 0; l < p->nl; ++l)
      if (p->has_drop[l] && u_d) {
        A.u[l] = u_d + (size_t)i * noise + (size_t)p->cfg.M * p->noise_off[l];
        A.bvar[l] = bvar_d + (size_t)i * noise + (size_t)p->cfg.M * p->noise_off[l];
      }
    T.loss_out = loss_hist_d ? loss_hist_d + (size_t)3 * i : loss_out_d;
    bnn_fwd_bwd_launch(p, A, ws, s);
    if (p->has_rule) {
      static_cast<BnnTailArgs&>(TR) = T;
      hipLaunchKernelGGL(p->kern.tail_rule, dim3(p->units), dim3(PM_BNT_NT), 0, s, TR);
    } else {
      hipLaunchKernelGGL(p->kern.tail, dim3(p->units), dim3(PM_BNT_NT), 0, s, T);
    }
  }
  if (loss_hist_d)
    HIPCHK(hipMemcpyAsync(loss_out_d, loss_hist_d + (size_t)3 * (n_steps - 1), 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIPCHK(hipGetLastError());
  return 0;
}
