// aomarl_capi_stages.hip -- part of the C ABI implementation (included by aomarl_capi.hip, one translation unit):
// the per-stage entry points: DM shapes, raytraces, WFS image / centroids, controller, target PSF / Strehl (A3 - A10).
// ---------------------------------------------------------------- DMs
// skip_stack: leave the stack-array planes alone (their phase will be evaluated from st->voltage
// inside the one-pass frame kernel); the tip-tilt slot (commands + pivot) is always refreshed
static int dm_shape_impl(aomarl_ctx *c, aomarl_state *st, int b, int n, const float *volts,
                         bool skip_stack, void *stream) {
  const float *v = volts ? volts : st->voltage + (size_t)b * st->ld_actu;
  const int ldv = volts ? c->sys.nactu : st->ld_actu;
  DevState ds = dev_state(st);
  for (int k = 0; k < c->ndm; k++) {
    const DevDm &D = c->sys.dms[k];
    const int np = D.dim * D.dim;
    if (D.type == AOMARL_DM_TT)
      hipLaunchKernelGGL(k_dm_shape, dim3(1, n), dim3(64), 0, (hipStream_t)stream, c->sys, ds, b, k, v, ldv);
    else if (skip_stack)
      continue;
    else if (D.sep && !c->force_generic_dm)
      hipLaunchKernelGGL(k_dm_shape_sep, dim3((D.dim + DMS_TX - 1) / DMS_TX, (D.dim + DMS_TY - 1) / DMS_TY, n),
                         dim3(256), 0, (hipStream_t)stream, c->sys, ds, b, k, v, ldv);
    else
      hipLaunchKernelGGL(k_dm_shape, dim3((np + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, c->sys, ds, b, k, v, ldv);
    LAUNCHCHK();
  }
  return 0;
}

int aomarl_comp_dm_shape(aomarl_ctx *c, aomarl_state *st, int b, int n, const float *volts, void *stream) {
  int rc = check_range(c, st, b, n);
  if (rc) return rc;
  if (n == 0) return 0;
  return dm_shape_impl(c, st, b, n, volts, false, stream);
}

int aomarl_dm_from_voltage_available(aomarl_ctx *c) {
  return c && c->sys.fused_ok && c->sys.otf_ok && !c->force_unfused_frame ? 1 : 0;
}

int aomarl_get_dm_shape(aomarl_ctx *c, aomarl_state *st, int b, int n, int k, float *dst, void *stream) {
  int rc = check_range(c, st, b, n);
  if (rc) return rc;
  if (k < 0 || k >= c->ndm || !dst) return fail("get_dm_shape: bad argument");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_get_dm_shape, dim3(256, n), dim3(256), 0, (hipStream_t)stream, c->sys, dev_state(st), b, k, dst);
  LAUNCHCHK();
  return 0;
}

int aomarl_set_option(aomarl_ctx *c, const char *name, int value) {
  if (!name) return fail("set_option: null argument");
  g_cfg_epoch++;
  if (c) c->cfg_epoch++;
  if (!strcmp(name, "gemm_kgroups")) {          // process-wide, no context needed
    if (value != 0 && value != 1 && value != 2 && value != 4) return fail("gemm_kgroups: 0, 1, 2 or 4");
    g_gemm_kgroups = value;
    return 0;
  }
  if (!strcmp(name, "gemm_xcd_map")) { g_gemm.xcd = value != 0; return 0; }   // process-wide
  if (!strcmp(name, "gemm_target_blocks")) { g_gemm.target_blocks = value > 0 ? value : 0; return 0; }   // process-wide
  if (!strcmp(name, "gemm_split_f16")) { g_gemm.split_f16 = value != 0; return 0; }          // process-wide
  if (!strcmp(name, "precision")) return aomarl_set_precision(value);                        // process-wide
  if (!c) return fail("set_option: null context");
  if (!strcmp(name, "force_generic_dm")) { c->force_generic_dm = value != 0; return 0; }
  if (!strcmp(name, "force_valu_target")) { c->force_valu_target = value != 0; return 0; }
  if (!strcmp(name, "defer_dm_shape")) { c->defer_dm_shape = value != 0; return 0; }
  if (!strcmp(name, "frame_pipeline")) {
    if (c->pipe.active) return fail("frame_pipeline: a frame is in flight (reset first)");
    c->pipe_enabled = value != 0; return 0;
  }
  if (!strcmp(name, "small_move")) { c->small_move = value != 0; return 0; }
  if (!strcmp(name, "small_chain")) { c->small_chain = value != 0; return 0; }
  if (!strcmp(name, "renew_frame_stream")) {
    // the frame pipeline's stream, anew: the runtime deals its hardware queues out as streams come, and a frame stream
    // that shares one with another stream of the step serialises the pipelined order (VecAoEnv's probe asks for this)
    auto &P = c->pipe;
    if (P.active) return fail("renew_frame_stream: a frame is in flight (reset first)");
    if (P.fstream) {
      HIPCHK(hipStreamSynchronize(P.fstream));
      HIPCHK(hipStreamDestroy(P.fstream));
      P.fstream = nullptr;
      HIPCHK(hipStreamCreateWithFlags(&P.fstream, hipStreamNonBlocking));
    }
    return 0;
  }
  if (!strcmp(name, "residual_shortcut")) {
    if (value && (!c->s2m || c->s2m_nmodes < 1)) return fail("residual_shortcut: no v2m . cmat matrix (aomarl_set_slopes2modes)");
    c->residual_shortcut = value != 0;
    return 0;
  }
  if (!strcmp(name, "reset_streams")) { c->reset_streams = value < 1 ? 1 : (value > 4 ? 4 : value); return 0; }
  if (!strcmp(name, "reset_prefetch_whole")) { c->reset_prefetch_whole = value != 0; return 0; }
  if (!strcmp(name, "extrude_unfused")) { c->no_extrude_sg = value != 0; return 0; }
  if (!strcmp(name, "reset_untransposed")) { c->reset_untransposed = value != 0; return 0; }
  if (!strcmp(name, "time_frame_kernel")) {
    // value = number of launches to keep event pairs for (0: off)
    c->time_fw = value > 0;
    { const int rrc = fw_ev_rewind(c); if (rrc) return rrc; }
    while (c->fw_ev.size() < 2 * (size_t)std::max(value, 0)) {
      hipEvent_t e;
      HIPCHK(hipEventCreate(&e));
      c->fw_ev.push_back(e);
    }
    return 0;
  }
  if (!strcmp(name, "prefetch_atmos")) { c->prefetch_atmos = value != 0; return 0; }
  if (!strcmp(name, "subpixel_flow")) { c->subpixel_flow = value != 0; return 0; }
  if (!strcmp(name, "graph_step")) { c->graph_step = value != 0; return 0; }
  if (!strcmp(name, "fused_debug")) { c->fused_debug = value; return 0; }
  if (!strcmp(name, "force_f32_dft")) { c->dft_mode = value < 0 ? -1 : (value != 0 ? 0 : 1); return 0; }
  if (!strcmp(name, "force_unfused_frame")) { c->force_unfused_frame = value != 0; return 0; }
  if (!strcmp(name, "force_generic_spot")) { c->force_generic_spot = value != 0; return 0; }
  if (!strcmp(name, "force_generic_target")) { c->force_generic_target = value != 0; return 0; }
  return fail("set_option: unknown option %s", name);
}

// ---------------------------------------------------------------- raytrace (unfused API)
// the static description with the layer windows moved by the wind accumulators' remainder ("subpixel_flow")
static DevSys traced_sys(const aomarl_ctx *c) {
  DevSys sy = c->sys;
  if (c->subpixel_flow)
    for (int l = 0; l < c->nlayers; l++) {
      sy.layers[l].wxo += c->frac_x[l]; sy.layers[l].txo += c->frac_x[l];
      sy.layers[l].wyo += c->frac_y[l]; sy.layers[l].tyo += c->frac_y[l];
    }
  return sy;
}

int aomarl_raytrace_wfs(aomarl_ctx *c, aomarl_state *st, int b, int n, int flags, void *stream) {
  int rc = check_range(c, st, b, n);
  if (rc) return rc;
  rc = atmos_wait_pending(c, stream);
  if (rc) return rc;
  if (!st->wfs_phase) return fail("raytrace_wfs needs st->wfs_phase");
  if (n == 0) return 0;
  const int np = c->sys.n * c->sys.n;
  hipLaunchKernelGGL(k_raytrace<false>, dim3((np + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, traced_sys(c), dev_state(st), b, flags);
  LAUNCHCHK();
  return 0;
}

int aomarl_raytrace_target(aomarl_ctx *c, aomarl_state *st, int b, int n, int flags, void *stream) {
  int rc = check_range(c, st, b, n);
  if (rc) return rc;
  rc = atmos_wait_pending(c, stream);
  if (rc) return rc;
  if (!st->tar_phase) return fail("raytrace_target needs st->tar_phase");
  if (n == 0) return 0;
  const int np = c->sys.pupdiam * c->sys.pupdiam;
  hipLaunchKernelGGL(k_raytrace<true>, dim3((np + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, traced_sys(c), dev_state(st), b, flags);
  LAUNCHCHK();
  return 0;
}

// ---------------------------------------------------------------- WFS
__global__ void k_inc_u32(uint32_t *p, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] += 1u;
}

int aomarl_comp_image(aomarl_ctx *c, aomarl_state *st, int b, int n, int flags, void *stream) {
  int rc = check_range(c, st, b, n);
  if (rc) return rc;
  rc = atmos_wait_pending(c, stream);
  if (rc) return rc;
  if (n == 0) return 0;
  SpotQuery q;
  q.from_buf = flags & AOMARL_IMG_FROM_PHASE_BUFFER;
  q.noise = (flags & AOMARL_IMG_NOISE) && c->sys.noise >= 0.f;
  q.cube = flags & AOMARL_IMG_WRITE_BINCUBE;
  q.cog = flags & AOMARL_IMG_COG;
  q.no_atmos = flags & AOMARL_IMG_NO_ATMOS; q.no_dms = flags & AOMARL_IMG_NO_DMS;
  q.force_generic_spot = c->force_generic_spot; q.production_layout = c->production_layout;
  q.nlayers = c->nlayers; q.nvalid = c->sys.nvalid; q.n = n;
  q.has_wfs_phase = st->wfs_phase != nullptr; q.has_bincube = st->bincube != nullptr;
  q.wfs_all_int = c->sys.wfs_all_int;
  const SpotPlan p = plan_spot(q);
  if (p.refusal != SPOT_OK) return fail("%s", spot_refusal_text(p.refusal));
  hipStream_t s = (hipStream_t)stream;
  rc = launch_spot(p, c->sys, dev_state(st), b, s);                // (aomarl_wfs.hip)
  if (rc) return rc;
  hipLaunchKernelGGL(k_inc_u32, dim3((n + 255) / 256), dim3(256), 0, s, st->frame + b, n);
  LAUNCHCHK();
  return 0;
}

int aomarl_do_centroids(aomarl_ctx *c, aomarl_state *st, int b, int n, void *stream) {
  int rc = check_range(c, st, b, n);
  if (rc) return rc;
  if (!st->bincube) return fail("do_centroids needs st->bincube");
  if (n == 0) return 0;
  return launch_cog(c->sys, dev_state(st), b, n, (hipStream_t)stream);
}

int aomarl_slopes_geom(aomarl_ctx *c, aomarl_state *st, int b, int n, void *stream) {
  int rc = check_range(c, st, b, n);
  if (rc) return rc;
  if (!st->wfs_phase) return fail("slopes_geom needs st->wfs_phase");
  if (n == 0) return 0;
  return launch_slopes_geom(c->sys, dev_state(st), b, n, (hipStream_t)stream);
}

// ---------------------------------------------------------------- controller
// modal gains (aomarl_set_modal_gains): the residual modes of rows [b, b + n), scaled in place by
// (gain or that environment's gain) * mgain[row or 0][m]
__global__ void k_mgain_scale(float *__restrict__ modes, int ldm, int nm, float gain, const float *__restrict__ env_gain,
                              const float *__restrict__ mgain, int mg_rows, int env_begin) {
  const int r = blockIdx.y, m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= nm) return;
  const int e = env_begin + r;
  const float g = env_gain ? env_gain[e] : gain;
  modes[(long long)r * ldm + m] *= g * mgain[(long long)(mg_rows > 1 ? e : 0) * nm + m];
}

// do_control under modal gains: err as ever (no integration in actuator space), then
// com += m2v . (gain * mgain (.) e),  e = -s2m . slopes
static int do_control_modal(aomarl_ctx *c, aomarl_state *st, int b, int n, void *stream) {
  int rc = mgain_check(c, st->nenv, "do_control");
  if (rc) return rc;
  if (!c->v2m || !c->m2v) return fail("do_control: modal gains are set (aomarl_set_modal_gains) but no modal basis (aomarl_set_modal)");
  if (!c->s2m || c->s2m_nmodes != c->nmodes)
    return fail("do_control: modal gains are set (aomarl_set_modal_gains): the integrator runs in Btt coordinates and needs "
                "the slopes-to-modes matrix of these %d modes (aomarl_set_slopes2modes)", c->nmodes);
  if (c->env_gain && c->env_gain_n != st->nenv)
    return fail("do_control: %d per-environment gains set, the state has %d environments", c->env_gain_n, st->nenv);
  // an on-line optimiser is attached with this state: it sees every frame whole.  A call with gain 0 (err alone, nothing
  // integrated: how callers refresh err) is not a frame of the loop and does not feed it.
  aomarl_modopti_online *mo = c->mo && c->mo_voltage == st->voltage && (c->gain != 0.f || c->env_gain) ? c->mo : nullptr;
  if (mo) {
    if (b != 0 || n != st->nenv)
      return fail("do_control: an on-line modal-gain optimiser is attached (aomarl_modopti_online_attach): the partial "
                  "environment range [%d, %d) of %d cannot feed it", b, b + n, st->nenv);
    if (c->env_gain) return fail("do_control: an on-line modal-gain optimiser is attached: per-environment scalar gains (aomarl_set_env_gains) are not supported");
    if (!(c->gain > 0.f)) return fail("do_control: an on-line modal-gain optimiser is attached: gain = %g must be positive", (double)c->gain);
    if (c->pipe.active) return fail("do_control: an on-line modal-gain optimiser is attached and a pipelined frame is in flight");
  }
  // a predictor attached with this state replaces the integration; the same rule for a call with gain 0
  aomarl_predictor *pr = c->pred && c->pred_voltage == st->voltage && (c->gain != 0.f || c->env_gain) ? c->pred : nullptr;
  if (pr) {
    if (b != 0 || n != st->nenv)
      return fail("do_control: a modal predictor is attached (aomarl_predictor_attach): the partial environment range "
                  "[%d, %d) of %d cannot feed it", b, b + n, st->nenv);
    if (c->env_gain) return fail("do_control: a modal predictor is attached: per-environment scalar gains (aomarl_set_env_gains) are not supported");
    if (c->pipe.active) return fail("do_control: a modal predictor is attached and a pipelined frame is in flight");
  }
  hipStream_t s = (hipStream_t)stream;
  const int na = c->sys.nactu, nsl = c->sys.nslope, nm = c->nmodes;
  Work w = work_layout(c, st->nenv);
  const float *slopes = st->slopes + (size_t)b * nsl;
  GemmArgs ge(n, na, nsl, -1.0f, slopes, nsl, c->cmat, c->ld_cmat, 0.0f, st->err + (size_t)b * st->ld_actu, st->ld_actu, s);
  ge.ws = st->work + w.GEMM; ge.ws_floats = w.gemm_floats; ge.min_chunk = 288;
  ge.fast = true; ge.sb = c->cmat_scale;
  launch_gemm_nt(ge);
  LAUNCHCHK();
  float *modes = st->work + w.MODES + (size_t)b * w.ldm;
  GemmArgs gs(n, nm, nsl, -1.0f, slopes, nsl, c->s2m, c->ld_cmat, 0.0f, modes, w.ldm, s);
  gs.ws = st->work + w.GEMM; gs.ws_floats = w.gemm_floats; gs.min_chunk = 288;
  gs.fast = true; gs.sb = c->s2m_scale;
  launch_gemm_nt(gs);
  LAUNCHCHK();
  if (mo || pr) {                    // x = e + v2m . voltage, the pseudo-open-loop modes, before e is scaled
    GemmArgs gp(n, nm, na, 1.0f, st->voltage, st->ld_actu, c->v2m, c->ld_v2m, 0.0f, mo ? mo_online_p(mo) : pred_p(pr), nm, s);
    gp.ws = st->work + w.GEMM; gp.ws_floats = w.gemm_floats; gp.min_chunk = 288;
    gp.fast = true; gp.sb = c->v2m_scale;                      /* volts */
    launch_gemm_nt(gp);
    LAUNCHCHK();
    rc = mo ? mo_online_pol(mo, modes, w.ldm, s) : mo_pol(modes, w.ldm, pred_p(pr), n, nm, pred_x(pr), s);
    if (rc) return rc;
  }
  float *com = st->com + (size_t)b * st->ld_actu;
  if (pr) {                          // c = theta . (x[t], x[t-1], ...) written over e, then com = m2v . c: nothing is integrated
    rc = pred_frame(pr, modes, w.ldm, s);
    if (rc) return rc;
    GemmArgs gc(n, na, nm, 1.0f, modes, w.ldm, c->m2v, c->ld_m2v, 0.0f, com, st->ld_actu, s);
    gc.ws = st->work + w.GEMM; gc.ws_floats = w.gemm_floats; gc.min_chunk = 288;
    gc.fast = true; gc.sa = 16.f; gc.sb = c->m2v_scale;        /* Btt coordinates x 2^4 */
    launch_gemm_nt(gc);
    LAUNCHCHK();
    return 0;
  }
  hipLaunchKernelGGL(k_mgain_scale, dim3((nm + 255) / 256, n), dim3(256), 0, s, modes, w.ldm, nm, c->gain, c->env_gain,
                     c->mgain, c->mgain_rows, b);
  LAUNCHCHK();
  GemmArgs gm(n, na, nm, 1.0f, modes, w.ldm, c->m2v, c->ld_m2v, 1.0f, com, st->ld_actu, s);
  gm.ws = st->work + w.GEMM; gm.ws_floats = w.gemm_floats; gm.min_chunk = 288;
  gm.fast = true; gm.sa = 16.f; gm.sb = c->m2v_scale;        /* Btt coordinates x 2^4 */
  launch_gemm_nt(gm);
  LAUNCHCHK();
  if (mo) {
    if (c->mo_used_stale) {          // the frame behind an apply: these are now the gains the last do_control used
      HIPCHK(hipMemcpyAsync(c->mo_mgain_used, c->mgain, sizeof(float) * (size_t)c->mgain_rows * (size_t)c->mgain_nm,
                            hipMemcpyDeviceToDevice, s));
      c->mo_used_stale = false;
    }
    bool applied = false;
    rc = mo_online_advance(mo, c->mgain, c->gain, s, &applied);      // the bank / the apply, where the schedule says so
    if (rc) return rc;
    c->mo_used_stale = applied;
  }
  return 0;
}

int aomarl_do_control(aomarl_ctx *c, aomarl_state *st, int b, int n, void *stream) {
  int rc = check_range(c, st, b, n);
  if (rc) return rc;
  if (!c->cmat) return fail("do_control: no command matrix (aomarl_set_cmat)");
  if (n == 0) return 0;
  if (c->mgain) return do_control_modal(c, st, b, n, stream);
  hipStream_t s = (hipStream_t)stream;
  const int na = c->sys.nactu, nsl = c->sys.nslope;
  // err[env][a] = - sum_s slopes[env][s] cmat[a][s]
  Work w = work_layout(c, st->nenv);
  GemmEpi ep = {};
  if (c->env_gain && c->env_gain_n != st->nenv)
    return fail("do_control: %d per-environment gains set, the state has %d environments", c->env_gain_n, st->nenv);
  ep.mode = 1; ep.com = st->com + (size_t)b * st->ld_actu; ep.ldcom = st->ld_actu; ep.gain = c->gain;
  ep.gain_row = c->env_gain ? c->env_gain + b : nullptr;
  GemmArgs ga(n, na, nsl, -1.0f, st->slopes + (size_t)b * nsl, nsl, c->cmat, c->ld_cmat, 0.0f,
              st->err + (size_t)b * st->ld_actu, st->ld_actu, s);
  ga.ws = st->work + w.GEMM; ga.ws_floats = w.gemm_floats; ga.epi = &ep; ga.min_chunk = 288;
  ga.fast = true; ga.sb = c->cmat_scale;                     /* slopes (arcsec): unscaled, saturation only beyond 65504" */
  const bool fused = launch_gemm_nt(ga).epi_done;
  LAUNCHCHK();
  if (!fused) {
    hipLaunchKernelGGL(k_integrate, dim3((na + 255) / 256, n), dim3(256), 0, s, st->com, st->err, na, st->ld_actu, c->gain, b, c->env_gain);
    LAUNCHCHK();
  }
  return 0;
}

int aomarl_set_com(aomarl_ctx *c, aomarl_state *st, int b, int n, const float *com, void *stream) {
  int rc = check_range(c, st, b, n);
  if (rc) return rc;
  if (!com) return fail("set_com: null command");
  if (n == 0) return 0;
  const int na = c->sys.nactu;
  hipLaunchKernelGGL(k_copy_rows, dim3((na + 255) / 256, n), dim3(256), 0, (hipStream_t)stream,
                     st->com + (size_t)b * st->ld_actu, st->ld_actu, com, na, na);
  LAUNCHCHK();
  return 0;
}

int aomarl_volts2modes(aomarl_ctx *c, aomarl_state *st, int nrows, const float *vec, int ldvec,
                       float *modes, void *stream) {
  if (!c || !c->v2m) return fail("volts2modes: no modal basis (aomarl_set_modal)");
  if (!vec || !modes) return fail("volts2modes: null argument");
  if (ldvec < c->sys.nactu) return fail("volts2modes: ldvec < nactu");
  float *ws = nullptr;
  size_t wsn = 0;
  if (st && st->work) { Work w = work_layout(c, st->nenv); ws = st->work + w.GEMM; wsn = w.gemm_floats; }
  GemmArgs ga(nrows, c->nmodes, c->sys.nactu, 1.0f, vec, ldvec, c->v2m, c->ld_v2m, 0.0f, modes, c->nmodes, (hipStream_t)stream);
  ga.ws = ws; ga.ws_floats = wsn; ga.min_chunk = 288;
  ga.fast = true; ga.sb = c->v2m_scale;                      /* volts */
  launch_gemm_nt(ga);
  LAUNCHCHK();
  return 0;
}

int aomarl_slopes2modes(aomarl_ctx *c, aomarl_state *st, int b, int n, float *modes, void *stream) {
  int rc = check_range(c, st, b, n);
  if (rc) return rc;
  if (!c->s2m || c->s2m_nmodes < 1) return fail("slopes2modes: no matrix (aomarl_set_slopes2modes)");
  if (!modes) return fail("slopes2modes: null output");
  if (n == 0) return 0;
  Work w = work_layout(c, st->nenv);
  const int nsl = c->sys.nslope, ld = (nsl + 3) & ~3;
  // residual modes = v2m . err = -(v2m . cmat) . slopes
  GemmArgs ga(n, c->s2m_nmodes, nsl, -1.0f, st->slopes + (size_t)b * nsl, nsl, c->s2m, ld, 0.0f, modes, c->s2m_nmodes,
              (hipStream_t)stream);
  ga.ws = st->work + w.GEMM; ga.ws_floats = w.gemm_floats; ga.min_chunk = 288;
  ga.fast = true; ga.sb = c->s2m_scale;                      /* slopes (arcsec), unscaled */
  launch_gemm_nt(ga);
  LAUNCHCHK();
  return 0;
}

int aomarl_rl_control(aomarl_ctx *c, aomarl_state *st, int b, int n, const float *action, void *stream) {
  int rc = check_range(c, st, b, n);
  if (rc) return rc;
  if (!c->v2m || !c->m2v) return fail("rl_control: no modal basis (aomarl_set_modal)");
  if (c->nact <= 0) return fail("rl_control: no action modes set");
  if (!action) return fail("rl_control: null action");
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  Work w = work_layout(c, st->nenv);
  float *modes = st->work + w.MODES;
  const int na = c->sys.nactu, nm = c->nmodes;
  float *com = st->com + (size_t)b * st->ld_actu;
  GemmEpi ep = {};
  ep.mode = 2; ep.action = action; ep.nact = c->nact; ep.amode_inv = c->amode_inv; ep.freedom = c->freedom;
  GemmArgs gv(n, nm, na, 1.0f, com, st->ld_actu, c->v2m, c->ld_v2m, 0.0f, modes, w.ldm, s);
  gv.ws = st->work + w.GEMM; gv.ws_floats = w.gemm_floats; gv.epi = &ep; gv.min_chunk = 288;
  gv.fast = true; gv.sb = c->v2m_scale;                      /* volts */
  const bool fused = launch_gemm_nt(gv).epi_done;
  LAUNCHCHK();
  if (!fused) {
    hipLaunchKernelGGL(k_modal_add, dim3((c->nact + 255) / 256, n), dim3(256), 0, s, modes, w.ldm, action, c->nact, c->amodes, c->freedom);
    LAUNCHCHK();
  }
  GemmArgs gm(n, na, nm, 1.0f, modes, w.ldm, c->m2v, c->ld_m2v, 0.0f, com, st->ld_actu, s);
  gm.ws = st->work + w.GEMM; gm.ws_floats = w.gemm_floats; gm.min_chunk = 288;
  gm.fast = true; gm.sa = 16.f; gm.sb = c->m2v_scale;        /* Btt coordinates x 2^4 */
  launch_gemm_nt(gm);
  LAUNCHCHK();
  return 0;
}

// modes = m0 + g * m1 (+ action on the action modes), written to the GEMM operand and to modes_out
__global__ void k_modal_compose(int nm, const float *__restrict__ m0, const float *__restrict__ m1,
                                float g, const float *__restrict__ action, int nact,
                                const int32_t *__restrict__ amode_inv,
                                const float *__restrict__ freedom, float *__restrict__ modes, int ldm,
                                float *__restrict__ modes_out) {
  const int r = blockIdx.y, m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= nm) return;
  float v = m0[(long long)r * nm + m] + g * m1[(long long)r * nm + m];
  if (action) {
    const int j = amode_inv[m];
    if (j >= 0) v += action[(long long)r * nact + j] * freedom[m];
  }
  modes[(long long)r * ldm + m] = v;
  if (modes_out) modes_out[(long long)r * nm + m] = v;
}

// k_modal_compose and k_agent_rewards side by side in one launch (blocks beyond the compose range: one
// per agent, first wave): both read the residual modes, neither reads what the other writes
__global__ __launch_bounds__(256) void k_compose_rewards(int nm, const float *__restrict__ m0, const float *__restrict__ m1,
                                                         float g, const float *__restrict__ action, int nact,
                                                         const int32_t *__restrict__ amode_inv,
                                                         const float *__restrict__ freedom, float *__restrict__ modes, int ldm,
                                                         float *__restrict__ modes_out, int cx, int n_agents,
                                                         const int32_t *__restrict__ lohi, float factor,
                                                         float *__restrict__ rew) {
  const int r = blockIdx.y;
  if ((int)blockIdx.x >= cx) {
    if (threadIdx.x >= 64) return;
    const int a = blockIdx.x - cx, lane = threadIdx.x;
    const int lo = lohi[2 * a], hi = lohi[2 * a + 1];
    float s = 0.f;
    for (int m = lo + lane; m < hi; m += 64) { const float v = m1[(long long)r * nm + m]; s += v * v; }
    s = wave_sum(s);
    if (lane == 0) rew[(long long)r * n_agents + a] = -factor * s / (float)(hi - lo);
    return;
  }
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= nm) return;
  float v = m0[(long long)r * nm + m] + g * m1[(long long)r * nm + m];
  if (action) {
    const int j = amode_inv[m];
    if (j >= 0) v += action[(long long)r * nact + j] * freedom[m];
  }
  modes[(long long)r * ldm + m] = v;
  if (modes_out) modes_out[(long long)r * nm + m] = v;
}

// k_modal_compose under modal gains (aomarl_set_modal_gains): modes = m0 + (g * mgain[m]) * m1, in that order -- with
// mgain = 1 the product g * 1 is g and the rest is k_modal_compose's expression: the same bits
__global__ void k_modal_compose_mgain(int nm, const float *__restrict__ m0, const float *__restrict__ m1,
                                      float g, const float *__restrict__ mgain, int mg_rows, int env_begin,
                                      const float *__restrict__ action, int nact,
                                      const int32_t *__restrict__ amode_inv,
                                      const float *__restrict__ freedom, float *__restrict__ modes, int ldm,
                                      float *__restrict__ modes_out) {
  const int r = blockIdx.y, m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= nm) return;
  const float gm = g * mgain[(long long)(mg_rows > 1 ? env_begin + r : 0) * nm + m];
  float v = m0[(long long)r * nm + m] + gm * m1[(long long)r * nm + m];
  if (action) {
    const int j = amode_inv[m];
    if (j >= 0) v += action[(long long)r * nact + j] * freedom[m];
  }
  modes[(long long)r * ldm + m] = v;
  if (modes_out) modes_out[(long long)r * nm + m] = v;
}

int aomarl_rl_control_modes(aomarl_ctx *c, aomarl_state *st, int b, int n, const float *m0,
                            const float *m1, float g, const float *action, float *modes_out,
                            void *stream) {
  int rc = check_range(c, st, b, n);
  if (rc) return rc;
  if (!c->v2m || !c->m2v) return fail("rl_control_modes: no modal basis (aomarl_set_modal)");
  // a predictor attached with this state: modes = c of the last frame (+ the action); m0, m1 and g are not read
  const float *pc = c->pred && c->pred_voltage == st->voltage ? pred_c(c->pred) + (size_t)b * c->nmodes : nullptr;
  if (!pc && (!m0 || !m1)) return fail("rl_control_modes: null modal vectors");
  if (action && c->nact <= 0) return fail("rl_control_modes: no action modes set");
  if (c->mgain && (rc = mgain_check(c, st->nenv, "rl_control_modes"))) return rc;
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  Work w = work_layout(c, st->nenv);
  float *modes = st->work + w.MODES;
  const int na = c->sys.nactu, nm = c->nmodes;
  if (pc)                            // k_modal_compose's expression with m0 = c and g = 0: c + 0 * c
    hipLaunchKernelGGL(k_modal_compose, dim3((nm + 255) / 256, n), dim3(256), 0, s, nm, pc, pc, 0.f, action,
                       c->nact, c->amode_inv, c->freedom, modes, w.ldm, modes_out);
  else if (c->mgain)
    hipLaunchKernelGGL(k_modal_compose_mgain, dim3((nm + 255) / 256, n), dim3(256), 0, s, nm, m0, m1, g,
                       c->mo ? c->mo_mgain_used : c->mgain,      /* attached: the gains the last do_control used */
                       c->mgain_rows, b, action, c->nact, c->amode_inv, c->freedom, modes, w.ldm, modes_out);
  else
    hipLaunchKernelGGL(k_modal_compose, dim3((nm + 255) / 256, n), dim3(256), 0, s, nm, m0, m1, g, action,
                       c->nact, c->amode_inv, c->freedom, modes, w.ldm, modes_out);
  LAUNCHCHK();
  GemmArgs ga(n, na, nm, 1.0f, modes, w.ldm, c->m2v, c->ld_m2v, 0.0f, st->com + (size_t)b * st->ld_actu, st->ld_actu, s);
  ga.ws = st->work + w.GEMM; ga.ws_floats = w.gemm_floats; ga.min_chunk = 288;
  ga.fast = true; ga.sa = 16.f; ga.sb = c->m2v_scale;        /* Btt coordinates x 2^4 */
  launch_gemm_nt(ga);
  LAUNCHCHK();
  return 0;
}

int aomarl_apply_control(aomarl_ctx *c, aomarl_state *st, int b, int n, int comp_voltage, void *stream) {
  int rc = check_range(c, st, b, n);
  if (rc) return rc;
  if (n == 0) return 0;
  const DelayWeights dw = delay_weights(c->delay, false);
  const int na = c->sys.nactu;
  hipLaunchKernelGGL(k_delay, dim3((na + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, dev_state(st), na, st->ld_actu, dw.wa, dw.wb, dw.wc, b, comp_voltage & AOMARL_APPLY_COMP_VOLTAGE);
  LAUNCHCHK();
  const bool defer = (comp_voltage & AOMARL_APPLY_DEFER_STACK_SHAPE) && aomarl_dm_from_voltage_available(c);
  return dm_shape_impl(c, st, b, n, nullptr, defer, stream);
}

// ---------------------------------------------------------------- target
static int target_psf_impl(aomarl_ctx *c, aomarl_state *st, int b, int n, bool from_buf, void *stream) {
  if (!from_buf && atmos_wait_pending(c, stream)) return 1;
  if (psf_wait_pending(c, stream)) return 1;
  hipStream_t s = (hipStream_t)stream;
  Work w = work_layout(c, st->nenv);
  const int W = 2 * c->sys.hw;
  float *TR = st->work + w.TR + (size_t)b * c->sys.pupdiam * W * 2;
  float *TP = st->work + w.TPART + (size_t)b * w.nblk * 4;
  float *PEND = st->work + w.PEND + (size_t)b * (W * W + 4);
  TargetQuery q;
  q.hw = c->sys.hw; q.npsf = c->sys.npsf; q.pupdiam = c->sys.pupdiam; q.nlayers = c->nlayers;
  q.from_buf = from_buf; q.production_layout = c->production_layout;
  q.force_valu_target = c->force_valu_target; q.force_generic_target = c->force_generic_target;
  q.nblk = w.nblk; q.n = n;
  const TargetPlan p = plan_target(q);
  const int rc = launch_target_rows(p, c->sys, dev_state(st), b, TR, TP, s);       // (aomarl_target.hip)
  if (rc) return rc;
  return launch_target_finish(p.finish, c->sys, TR, TP, p.nblk, PEND, nullptr, n, s);
}

int aomarl_target_psf(aomarl_ctx *c, aomarl_state *st, int b, int n, void *stream) {
  int rc = check_range(c, st, b, n);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!c->sys.tar_all_int) {
    rc = aomarl_raytrace_target(c, st, b, n, AOMARL_TRACE_ATMOS | AOMARL_TRACE_DMS | AOMARL_TRACE_RESET, stream);
    if (rc) return rc;
    return target_psf_impl(c, st, b, n, true, stream);
  }
  return target_psf_impl(c, st, b, n, false, stream);
}

int aomarl_comp_strehl(aomarl_ctx *c, aomarl_state *st, int b, int n, void *stream) {
  int rc = check_range(c, st, b, n);
  if (rc) return rc;
  if (n == 0) return 0;
  rc = psf_wait_pending(c, stream);
  if (rc) return rc;
  Work w = work_layout(c, st->nenv);
  const int W = 2 * c->sys.hw;
  float *PEND = st->work + w.PEND + (size_t)b * (W * W + 4);
  return launch_strehl_commit(c->sys, dev_state(st), b, n, PEND, (hipStream_t)stream);
}

int aomarl_strehl_fit(aomarl_ctx *c, aomarl_state *st, int b, int n, void *stream) {
  if (!c || !st) return fail("strehl_fit: null ctx/state");
  if (b < 0 || n < 0 || b + n > st->nenv || !st->strehl || !st->le_img) return fail("strehl_fit: bad range / state");
  if (n == 0) return 0;
  return launch_strehl_fit_le(c->sys, dev_state(st), b, n, (hipStream_t)stream);
}
