// pcg_abi_cfg.hip -- configuration folding: a pcg_env_cfg into the plan's DevConst (build_devconst), its per-step table of
// wave-uniform values (lean_table) and its row of the kernel table (kernel_id_for).  No HIP calls.
#include "pcg_host.hpp"

namespace pcg {

// Validates cfg and fills the host DevConst.  No HIP calls: unit-testable without a GPU.
int build_devconst(const pcg_env_cfg* c, DevConst* d, int* cfg_nu_out) {
  if (!c || !d) return PCG_E_NULL;
  if (c->model_id < 0 || c->model_id >= PCG_MODEL_COUNT) return PCG_E_MODEL;
  if (c->integrator_id < 0 || c->integrator_id >= PCG_INT_COUNT) return PCG_E_MODEL;
  const bool user = c->model_id == PCG_MODEL_USER;
  Kernels ku = kernels(c->model_id);
  if (user) {  // sizes come from the cfg; the right-hand side from cfg.user_rhs_src
    ku.nx = c->nx; ku.na = c->na; ku.ndm = c->ndm; ku.nraw = c->n_params;
  }
  const Kernels& k = ku;
  const int nx = c->nx, na = c->na, ndm = c->ndm, nd = c->nd, nsp = c->nsp, ncon = c->ncon, nrew = c->nrew;
  if (user) {
    if (!c->user_rhs_src) return PCG_E_NULL;
    if (nx < 1 || nx > PCG_MAX_NX || na < 1 || na > PCG_MAX_NA || ndm < 0 || ndm > PCG_MAX_NDM) return PCG_E_DIM;
    if (c->n_params < 0 || c->n_params > PCG_MAX_USER_PARAMS) return PCG_E_DIM;
    if (c->nunc > 0) return PCG_E_UNSUPPORTED;
  } else if (c->user_rhs_src) {
    return PCG_E_UNSUPPORTED;
  }
  if (user) {
  } else if (k.dynamic) {
    if (nx < 1 || nx > k.nx || na < 1 || na > k.na || ndm != 0) return PCG_E_DIM;
    if (c->n_params != nx * nx + nx * na + nx) return PCG_E_DIM;
  } else {
    if (nx != k.nx || na != k.na) return PCG_E_DIM;
    if (ndm != 0 && ndm != k.ndm) return PCG_E_DIM;
    if (c->n_params != k.nraw) return PCG_E_DIM;
    // coupled_oscillators: the ring size is a structural parameter, only the reference default N = 10 is compiled
    if (c->model_id == PCG_MODEL_OSCILLATORS && (!c->params || c->params[0] != 10.0)) return PCG_E_UNSUPPORTED;
  }
  if (nd < 0 || nd > ndm || nsp < 0 || nsp > PCG_MAX_NSP || ncon < 0 || ncon > PCG_MAX_NCON) return PCG_E_DIM;
  const int nso = c->nsp_obs;
  const int nunc = c->nunc;
  if (nunc < 0 || nunc > PCG_MAX_NUNC) return PCG_E_DIM;
  if (nunc > 0 && (k.dynamic || !c->unc_index || !c->unc_pct)) return nunc > 0 && k.dynamic ? PCG_E_UNSUPPORTED : PCG_E_NULL;
  if (nunc > 0 && ndm > 0 && !c->d_param_index) return PCG_E_NULL;  // Q11: which parameter an unconfigured input reads
  if (nso != 0 && nso != nsp) return PCG_E_DIM;
  if (nd > 0 && nso != nsp) return PCG_E_UNSUPPORTED;
  if (nrew < 0 || nrew > PCG_MAX_NX) return PCG_E_DIM;
  if (c->N < 2 || c->N > PCG_MAX_N) return PCG_E_DIM;
  if (!(c->dt > 0.0) || !std::isfinite(c->dt)) return PCG_E_VALUE;
  if (c->integrator_id == PCG_INT_RK4 && c->substeps < 0) return PCG_E_VALUE;  // 0 = no integration (I/O probe)
  if ((c->integrator_id == PCG_INT_RK4G || c->integrator_id == PCG_INT_T5G) &&
      (c->substeps < 1 || !k.step[c->integrator_id][0][0][0] || c->nunc > 0))
    return c->substeps < 1 ? PCG_E_VALUE : PCG_E_UNSUPPORTED;  // models with a guard hook only
  if (c->integrator_id == PCG_INT_CV8 && (c->substeps < 1 || c->nunc > 0)) return c->substeps < 1 ? PCG_E_VALUE : PCG_E_UNSUPPORTED;
  if (c->integrator_id != PCG_INT_RK4 && (!(c->rtol > 0) || !(c->atol >= 0) || c->max_steps < 1))
    return PCG_E_VALUE;
  const int nobs = nx + nso + nd + nunc, cnu = na + ndm;
  if ((!c->params && !(user && c->n_params == 0)) || !c->x0 || !c->a_low || !c->a_high || !c->o_low || !c->o_high) return PCG_E_NULL;
  if (nsp && (!c->sp_index || !c->sp)) return PCG_E_NULL;
  if ((nsp || nrew) && !c->r_scale) return PCG_E_NULL;
  if (nrew && !c->rew_index) return PCG_E_NULL;
  if (nd && (!c->d_slot || !c->d_sched)) return PCG_E_NULL;
  if (ndm && !c->d_default) return PCG_E_NULL;
  if (ncon && !c->user_cons_src && (!c->con_A || !c->con_b)) return PCG_E_NULL;
  if ((c->user_cons_src || c->user_reward_src) && (k.dynamic || c->nunc > 0)) return PCG_E_UNSUPPORTED;
  if ((c->flags & PCG_F_A_DELTA) && (!c->a_act_low || !c->a_act_high || !c->a_0)) return PCG_E_NULL;
  if ((c->flags & PCG_F_NOISE) && !c->noise_pct) return PCG_E_NULL;
  if ((c->flags & PCG_F_GAUSS_DIST) && nd && (!c->d_sigma || !c->d_clip_lo || !c->d_clip_hi)) return PCG_E_NULL;

  std::memset(d, 0, sizeof(*d));
  double ddef[PCG_MAX_NDM] = {0, 0, 0, 0};
  if (user) {
    static_assert(PCG_MAX_USER_PARAMS <= sizeof(d->kp_big) / sizeof(double), "user parameters live in kp_big");
    for (int i = 0; i < c->n_params; ++i) d->kp_big[i] = c->params[i];
  } else {
    k.prep(c->params, nx, na, k.dynamic ? d->kp_big : d->kp, ddef);
  }
  for (int j = 0; j < k.ndm; ++j) d->d_default[j] = ndm ? c->d_default[j] : ddef[j];
  const bool norm_a = c->flags & PCG_F_NORMALISE_A, norm_o = c->flags & PCG_F_NORMALISE_O;
  const bool compat = c->flags & PCG_F_REF_COMPAT;
  for (int i = 0; i < na; ++i) {
    d->a_lo[i] = c->a_low[i];
    d->a_hi[i] = c->a_high[i];
    if (c->flags & PCG_F_A_DELTA) {
      d->a_act_lo[i] = c->a_act_low[i]; d->a_act_hi[i] = c->a_act_high[i]; d->a_0[i] = c->a_0[i];
    }
  }
  // the lean step's action map: the half widths folded here, for the whole plan or not at all (amap_fold, pcg_kernels.hpp)
  d->a_mode = norm_a ? PCG_AMAP_FOLDED : PCG_AMAP_NONE;
  for (int i = 0; i < na; ++i)
    if (norm_a && !amap_fold(d->a_lo[i], d->a_hi[i], &d->a_w[i])) d->a_mode = PCG_AMAP_EXACT;
  for (int i = 0; i < nobs; ++i) {
    const bool masked = (i < nx) && c->obs_mask && !c->obs_mask[i];
    if (masked) {
      d->omap[i] = OMap{0, 0, 0};
    } else if (norm_o) {
      if (!(c->o_high[i] > c->o_low[i])) return PCG_E_VALUE;
      d->omap[i] = OMap{c->o_low[i], 2.0 / (c->o_high[i] - c->o_low[i]), -1.0};
    } else {
      d->omap[i] = OMap{0, 1, 0};
    }
  }
  for (int i = 0; i < nsp; ++i) {
    if (c->sp_index[i] < 0 || c->sp_index[i] >= nx) return PCG_E_DIM;
    d->sp_index[i] = c->sp_index[i];
  }
  for (int i = 0; i < nrew; ++i) {
    if (c->rew_index[i] < 0 || c->rew_index[i] >= nx) return PCG_E_DIM;
    d->rew_index[i] = c->rew_index[i];
  }
  const int nrs = (c->flags & PCG_F_REWARD_BATCH) ? nrew : nsp;
  for (int i = 0; i < nrs; ++i) d->r_scale[i] = c->r_scale[i];
  if (c->flags & PCG_F_REWARD_TRACK) {
    // normalisation of the tracking reward is always by o_space / a_space (custom_reward.py:14-31), whether or
    // not the env normalises its observations / actions
    if ((c->flags & PCG_F_REWARD_BATCH) || nsp == 0) return PCG_E_UNSUPPORTED;
    if ((c->flags & PCG_F_REWARD_CRYST) && c->model_id != PCG_MODEL_CRYST) return PCG_E_UNSUPPORTED;
    if (c->rew_nbox < 0 || c->rew_nbox > PCG_MAX_RBOX) return PCG_E_DIM;
    if (c->rew_nbox > 0 && (!c->rew_box_index || !c->rew_box_lo || !c->rew_box_hi)) return PCG_E_NULL;
    if (nd > 0) return PCG_E_UNSUPPORTED;  // the reference broadcasts uk (Nu + Nd) against a_space (Nu) there
    for (int k = 0; k < nsp; ++k) {
      const int i = c->sp_index[k];
      const double w = c->o_high[i] - c->o_low[i];
      if (!(w != 0.0)) return PCG_E_VALUE;
      d->trk_lo[k] = c->o_low[i];
      d->trk_inv[k] = 1.0 / w;
    }
    for (int j = 0; j < na; ++j) {
      const double w = c->a_high[j] - c->a_low[j];
      if (!(w != 0.0)) return PCG_E_VALUE;
      d->act_lo[j] = c->a_low[j];
      d->act_inv[j] = 1.0 / w;
    }
    d->R_du = c->rew_R_du;
    d->R_u = c->rew_R_u;
    d->nbox = c->rew_nbox;
    for (int q = 0; q < c->rew_nbox; ++q) {
      const int i = c->rew_box_index[q];
      if (i < 0 || i >= nx) return PCG_E_DIM;
      const double w = c->o_high[i] - c->o_low[i];
      if (!(w != 0.0)) return PCG_E_VALUE;
      d->box_index[q] = i;
      d->box_lo[q] = c->o_low[i];
      d->box_inv[q] = 1.0 / w;
      d->box_lon[q] = (c->rew_box_lo[q] - c->o_low[i]) / w;
      d->box_hin[q] = (c->rew_box_hi[q] - c->o_low[i]) / w;
    }
  }
  if (c->flags & PCG_F_NOISE)
    for (int i = 0; i < nx; ++i) d->noise_pct[i] = c->noise_pct[i];
  for (int i = 0; i < nx + nso; ++i) d->x0[i] = c->x0[i];
  d->has_x0_unc = c->x0_unc ? 1 : 0;
  if (c->x0_unc)
    for (int i = 0; i < nx; ++i) d->x0_unc[i] = c->x0_unc[i];
  for (int i = 0; i < nd; ++i) {
    if (c->d_slot[i] < 0 || c->d_slot[i] >= ndm) return PCG_E_DIM;
    d->d_slot[i] = c->d_slot[i];
    if (c->flags & PCG_F_GAUSS_DIST) {
      d->d_sigma[i] = c->d_sigma[i]; d->d_lo[i] = c->d_clip_lo[i]; d->d_hi[i] = c->d_clip_hi[i];
    }
  }
  // constraint rows: cfg layout [state(nobs) | uk(cnu)] -> padded kernel layout; compat Q3 folded:
  //   state' = (s+1)*hs + lo = s*hs + (hs+lo)   (pcgym.py:601-608), input' likewise with a_space (:597-600)
  // the same quirk for user constraint expressions, as an affine map of the vectors they index
  for (int i = 0; i < PCG_MAX_NOBS; ++i) { d->q3_mul[i] = 1.0; d->q3_add[i] = 0.0; }
  for (int j = 0; j < KNU; ++j) { d->q3u_mul[j] = 1.0; d->q3u_add[j] = 0.0; }
  if (compat && norm_o)
    for (int i = 0; i < nobs; ++i) {
      const double hs = (c->o_high[i] - c->o_low[i]) / 2;
      d->q3_mul[i] = hs;
      d->q3_add[i] = hs + c->o_low[i];
    }
  if (compat && norm_a && c->user_cons_src) {
    if (cnu != na && na != 1) return PCG_E_UNSUPPORTED;  // the reference itself raises (broadcast error)
    for (int j = 0; j < cnu; ++j) {
      const int q = (na == 1) ? 0 : j;
      const double hs = (c->a_high[q] - c->a_low[q]) / 2;
      const int col = (j < na) ? j : k.na + (j - na);  // kernel-side u layout [NA | NDM]
      d->q3u_mul[col] = hs;
      d->q3u_add[col] = hs + c->a_low[q];
    }
  }
  for (int r = 0; r < (c->user_cons_src ? 0 : ncon); ++r) {
    const double* row = c->con_A + (size_t)r * (nobs + cnu);
    double b = c->con_b[r];
    for (int i = 0; i < nobs; ++i) {
      double coef = row[i];
      if (compat && norm_o) {
        const double hs = (c->o_high[i] - c->o_low[i]) / 2;
        b -= coef * (hs + c->o_low[i]);
        coef *= hs;
      }
      if (i >= nx + nso + nd) {  // uncertain-parameter slots cannot enter constraint rows
        if (coef != 0.0) return PCG_E_UNSUPPORTED;
        continue;
      }
      const int col = (i < nx) ? i : (i < nx + nso) ? PCG_MAX_NX + (i - nx) : PCG_MAX_NX + PCG_MAX_NSP + (i - nx - nso);
      d->con_A[r][col] = coef;
    }
    for (int j = 0; j < cnu; ++j) {
      double coef = row[nobs + j];
      if (compat && norm_a) {
        if (cnu != na && na != 1) return PCG_E_UNSUPPORTED;  // the reference itself raises (broadcast error)
        const int q = (na == 1) ? 0 : j;
        const double hs = (c->a_high[q] - c->a_low[q]) / 2;
        b -= coef * (hs + c->a_low[q]);
        coef *= hs;
      }
      const int col = PCG_MAX_NX + PCG_MAX_NSP + PCG_MAX_NDM + ((j < na) ? j : PCG_MAX_NA + (j - na));
      d->con_A[r][col] = coef;
    }
    d->con_b[r] = b;
  }
  d->nunc = nunc;
  if (!k.dynamic && !user)
    for (int i = 0; i < k.nraw && i < 32; ++i) d->raw[i] = c->params[i];
  for (int j = 0; j < nunc; ++j) {
    // index == nraw: an INERT entry (sampled at reset and observed, substituted into no model parameter) -- what the
    // reference does with empirical_distribution['x0'] (pcgym.py:311-316); empirical tables only
    const bool inert = (c->flags & PCG_F_UNC_EMPIRICAL) && c->unc_index[j] == k.nraw && k.nraw < 32;
    if ((c->unc_index[j] < 0 || c->unc_index[j] >= k.nraw) && !inert) return PCG_E_DIM;
    d->unc_index[j] = c->unc_index[j];
    d->unc_pct[j] = c->unc_pct[j];
    if (c->flags & PCG_F_UNC_EMPIRICAL) {
      if (!c->unc_emp || !c->unc_emp_off) return PCG_E_NULL;
      if (c->unc_emp_off[0] != 0 || c->unc_emp_off[j + 1] <= c->unc_emp_off[j] || c->unc_emp_off[j + 1] > PCG_MAX_EMP)
        return PCG_E_DIM;
      d->emp_off[j] = c->unc_emp_off[j];
      d->emp_off[j + 1] = c->unc_emp_off[j + 1];
    }
  }
  d->dt = c->dt;
  d->h = c->dt / (c->substeps > 0 ? c->substeps : 1);
  d->h2 = 0.5 * d->h;
  d->h6 = d->h / 6.0;
  d->rtol = c->rtol;
  d->dt_edge = c->dt * (1.0 - 1e-14);
  d->h_floor = 1e-13 * c->dt;
  // end-point error control of the Rosenbrock pairs (PCG_INT_RODAS4 / PCG_INT_RODAS5, pcgym_hip.h): exponent rate = ep_c x the
  // model's contraction rate
  if (is_ros_pair(c->integrator_id)) {
    if (!(c->ep_frac >= 0.0 && c->ep_frac <= 1.0) || c->ep_kmax < 0 || c->ep_kmax > 40) return PCG_E_VALUE;
    if (c->nunc > 0) return PCG_E_UNSUPPORTED;
    d->ep_kmax = c->ep_kmax;
    d->ep_c = c->ep_kmax > 0 ? c->ep_frac * 1.4426950408889634 : 0.0;
  }
  // cooperative rule (pcgym_hip.h: coop_thr): only where the model's kernels carry it
  d->coop_thr = 0.0;
  if (c->coop_thr != 0.0) {
    if (!(c->coop_thr > 0.0) || !std::isfinite(c->coop_thr)) return PCG_E_VALUE;
    if (!is_ros_pair(c->integrator_id) || user || !c->params || !kernels(kernel_id_for(c)).coop) return PCG_E_UNSUPPORTED;
    d->coop_thr = c->coop_thr;
  }
  d->atol = c->atol;
  d->nx = nx; d->na = na; d->ndm = ndm; d->nd = nd; d->nsp = nsp; d->nsp_obs = nso; d->ncon = ncon; d->nrew = nrew;
  d->N = c->N; d->substeps = c->substeps; d->max_steps = c->max_steps; d->nobs = nobs;
  d->flags = c->flags;
  if (cfg_nu_out) *cfg_nu_out = cnu;
  return PCG_OK;
}

// The wave-uniform values of every lock-stepped step t -> t + 1 (LeanStep, pcg_kernels.hpp), computed here once per plan
// with the operations the kernels used to repeat per tile: the observation slots through the folded OMap as one fused
// multiply-add of (v - lo), the schedule indices of pcgym.py:394,438,555 (quirks Q5, Q6) clamped to the last column.
std::vector<LeanStep> lean_table(const DevConst& d, const pcg_env_cfg* c) {
  const int N = d.N > 0 ? d.N : 1;
  std::vector<LeanStep> tab((size_t)N);
  for (int t = 0; t < N; ++t) {
    LeanStep& L = tab[(size_t)t];
    std::memset(&L, 0, sizeof(L));
    const int tc = t < N - 1 ? t : N - 1, tn = t + 1 < N - 1 ? t + 1 : N - 1;
    for (int k = 0; k < d.nsp && k < PCG_MAX_NSP; ++k) {
      L.spn[k] = c->sp[(size_t)k * N + tn];
      if (k < d.nsp_obs) {
        const OMap& m = d.omap[d.nx + k];
        L.osp[k] = std::fma(c->sp[(size_t)k * N + tc] - m.lo, m.sc, m.off);
      }
    }
    for (int j = 0; j < PCG_MAX_NDM; ++j) L.ud[j] = d.d_default[j];
    for (int k = 0; k < d.nd && k < PCG_MAX_NDM; ++k) {
      const double v = c->d_sched[(size_t)k * N + tn];
      const OMap& m = d.omap[d.nx + d.nsp_obs + k];
      L.od[k] = std::fma(v - m.lo, m.sc, m.off);
      const int slot = d.d_slot[k];
      if (slot >= 0 && slot < PCG_MAX_NDM) L.ud[slot] = v;
    }
  }
  return tab;
}

// eq_exponent == 2 (the reference default) selects the multiply-only instantiation of the extraction models;
// not when the exponent itself is one of the per-env uncertain parameters.
int kernel_id_for(const pcg_env_cfg* c) {
  int epos = -1, kid = c->model_id;
  if (c->model_id == PCG_MODEL_ME) { epos = 4; kid = PCG_KID_ME_SQ; }
  if (c->model_id == PCG_MODEL_ME_REACTIVE) { epos = 5; kid = PCG_KID_ME_REACTIVE_SQ; }
  if (epos < 0 || c->params[epos] != 2.0) return c->model_id;
  for (int j = 0; j < c->nunc; ++j)
    if (c->unc_index[j] == epos) return c->model_id;
  return kid;
}
}  // namespace pcg
