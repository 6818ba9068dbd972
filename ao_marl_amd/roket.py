"""ROKET error breakdown of the closed loop for batched environments (reference: guardians/roket_generalized_rl.py,
src/error_budget/error_budget_multiple_agents.py).

RoketBank          the native contributor filter bank and its modal moments (csrc/aomarl_roket.hip): the loop filters of
                   the seven contributors and the sums their covariance table is made of stay on the device -- the
                   reference's [n_iter][nactu] host histories do not scale to hundreds of environments.
cov_cor_moments    the reference's cov / cor table (cov_cor, :441-480) and the per-mode variances from those sums.
"""
import ctypes as C

import numpy as np

from . import attachments
from . import libaomarl as la

# the order of the reference's covariance table (cov_cor, :445-453), with the key names of save_in_hdf5 (:402-410)
CONTRIBUTORS = ("noise", "non linearity", "aliasing", "filtered modes", "bandwidth", "tomography", "zeta")
NC = 7
PAIRS = [(k, l) for k in range(NC) for l in range(k, NC)]
PAIR_INDEX = {p: i for i, p in enumerate(PAIRS)}


def cov_cor_moments(S1, S2, frames, with_zeta=True):
    """S1 [7][nmodes], S2 [28][nmodes] (pairs k <= l, k major), sums over `frames` frames of y_k = P x_k and
    y_k y_l -> (cov, cor, var): the reference's tables (7x7 with a policy, 6x6 without) and the per-mode covariance
    var [n][n][nmodes] they are the sums of (cov[i, j] = sum_m mean(y_i y_j) - mean(y_i) mean(y_j))."""
    S1, S2 = np.asarray(S1, dtype=np.float64), np.asarray(S2, dtype=np.float64)
    if frames < 1:
        raise ValueError("no frame was accumulated")
    n = NC if with_zeta else NC - 1
    nm = S1.shape[-1]
    var = np.zeros((n, n, nm))
    for i in range(n):
        for j in range(i, n):
            var[i, j] = var[j, i] = S2[PAIR_INDEX[(i, j)]] / frames - (S1[i] / frames) * (S1[j] / frames)
    cov = var.sum(axis=2)
    cor = np.zeros_like(cov)
    s = np.diag(cov).reshape(n, 1)
    sst = s.dot(s.T)
    ok = np.where(sst)
    cor[ok] = cov[ok] / np.sqrt(sst[ok])
    return cov, cor, var


class RoketBank(object):
    """aomarl_roket_* for `nenv` environments.  RD = cmat . imat [nactu][nactu], P [nmodes][nactu],
    Btt [nactu][nmodes] (host); delay = int(p_controllers[0].delay) + 1; inputs of step(): device tensors
    [nenv][>= nactu] with unit column stride and a common row stride (the state's ld_actu)."""

    def __init__(self, nenv, RD, P, Btt, g, gamma, nfiltered, delay, ld_actu=None, device="cuda:0"):
        import torch
        self.lib = la.load()
        self.device = torch.device(device)
        P = np.ascontiguousarray(P, dtype=np.float32)
        Btt = np.ascontiguousarray(Btt, dtype=np.float32)
        RD = np.ascontiguousarray(RD, dtype=np.float32)
        self.nmodes, self.nactu = P.shape
        if Btt.shape != (self.nactu, self.nmodes) or RD.shape != (self.nactu, self.nactu):
            raise ValueError("RD %s, P %s, Btt %s do not agree" % (RD.shape, P.shape, Btt.shape))
        self.nenv, self.ld_actu = int(nenv), int(ld_actu or self.nactu)
        self.nfiltered, self.delay, self.g, self.gamma = int(nfiltered), int(delay), float(g), float(gamma)
        d = la.RoketDesc()
        d.nenv, d.nactu, d.ld_actu, d.nmodes = self.nenv, self.nactu, self.ld_actu, self.nmodes
        d.nfiltered, d.delay, d.g, d.gamma = self.nfiltered, self.delay, self.g, self.gamma
        d.RD, d.P, d.Btt = la.fptr(RD), la.fptr(P), la.fptr(Btt)
        self.ptr = C.c_void_p()
        if not torch.cuda.is_available():
            raise la.AomarlError("RoketBank needs a GPU: there is no CPU fallback for the filter bank")
        with torch.cuda.device(self.device):
            la.check(self.lib.aomarl_roket_create(C.byref(d), C.byref(self.ptr)))

    def __del__(self):
        if getattr(self, "ptr", None):
            self.lib.aomarl_roket_destroy(self.ptr)
            self.ptr = None

    def _in(self, t, name, optional=False):
        if t is None:
            if optional:
                return None
            raise ValueError("%s is required" % name)
        if t.dim() != 2 or t.shape[0] != self.nenv or t.shape[1] < self.nactu or t.stride(1) != 1 or \
                t.stride(0) != self.ld_actu or str(t.dtype) != "torch.float32" or not t.is_cuda:
            raise ValueError("%s must be a float32 device tensor [%d][>= %d] with row stride %d" %
                             (name, self.nenv, self.nactu, self.ld_actu))
        return t.data_ptr()

    def step(self, derr, E, F, ageom, B, G=None, rl_com=None, accumulate=True):
        """Frame t (aomarl_roket_step).  G=None: G = B (coincident directions); rl_com=None: no policy."""
        la.check(self.lib.aomarl_roket_step(
                self.ptr, self._in(derr, "derr"), self._in(E, "E"), self._in(F, "F"), self._in(ageom, "ageom"),
                self._in(B, "B"), self._in(G, "G", True), self._in(rl_com, "rl_com", True), 1 if accumulate else 0,
                la.raw_stream(self.device)))

    def history(self):
        """(x [7][nenv][nactu], bufs [4][nenv][nactu]): the contributors of the last frame in CONTRIBUTORS' order, and
        its noise_buf, trunc_buf, tomo_buf, mod_com."""
        import torch
        x = torch.empty(NC, self.nenv, self.nactu, dtype=torch.float32, device=self.device)
        b = torch.empty(4, self.nenv, self.nactu, dtype=torch.float32, device=self.device)
        la.check(self.lib.aomarl_roket_history(self.ptr, x.data_ptr(), b.data_ptr(), la.raw_stream(self.device)))
        return x, b

    def moments(self):
        """(S1 [nenv][7][nmodes], S2 [nenv][28][nmodes], frames): float64 NumPy arrays."""
        import torch
        S1 = torch.empty(self.nenv, NC, self.nmodes, dtype=torch.float64, device=self.device)
        S2 = torch.empty(self.nenv, len(PAIRS), self.nmodes, dtype=torch.float64, device=self.device)
        n = C.c_longlong(0)
        la.check(self.lib.aomarl_roket_moments(self.ptr, S1.data_ptr(), S2.data_ptr(), C.byref(n),
                                               la.raw_stream(self.device)))
        return S1.cpu().numpy(), S2.cpu().numpy(), int(n.value)

    def reset(self):
        la.check(self.lib.aomarl_roket_reset(self.ptr))


# ---------------------------------------------------------------------------------------------- the breakdown
_REFUSED = ("frame_pipeline", ("screens_ahead", "the breakdown would trace the NEXT frame's atmosphere (geo=True builds "
                                                "it that way)"), "reset_prefetch",
            ("env_gains", "the loop filter gRD is one matrix for all environments"),
            ("modal_gains", "the loop filter gRD assumes the scalar integrator law"), "pure_delay_0",
            ("autoencoder", "the breakdown of a denoised sensor is not covered", NotImplementedError))


def _roket_supervisor(env):
    """The supervisor the breakdown runs on; refuses, naming the argument, every configuration in which the frame
    the loop measured is not the one its screens and mirrors stand on, or that the breakdown has no branch for."""
    sup = getattr(env, "supervisor", None)
    if sup is None or not hasattr(env, "rl_step"):
        raise TypeError("VecRoket: env must be a VecAoEnv")
    if getattr(env, "frame_pipeline", False) is not False:
        raise RuntimeError("VecRoket: the pipelined call order (frame_pipeline=%r) images frames one step ahead of "
                           "the chains; build the environment with frame_pipeline=False" % (env.frame_pipeline,))
    # (every attachment that senses: the breakdown's mirrors and its loop filter, gRD, are the Shack-Hartmann loop's)
    attachments.refuse(sup, "VecRoket", _REFUSED, [s for s, r in attachments.TABLE.items() if r.senses])
    if sup.geo is None:
        raise RuntimeError("VecRoket: the fitting term and B come from the geometric twin; build the environment "
                           "with geo=True")
    cfg = sup.config
    w, t = cfg.p_wfss[0], cfg.p_targets[0]
    if str(w.type).lower() != "sh":
        raise NotImplementedError("VecRoket: p_wfss[0].type = %r: Shack-Hartmann sensors only" % (w.type,))
    if str(cfg.p_centroiders[0].type).lower() != "cog":
        raise NotImplementedError("VecRoket: p_centroiders[0].type = %r: the thresholded-centroid branch "
                                  "(roket_generalized_rl.py:198-210) is not covered, plain cog only"
                                  % (cfg.p_centroiders[0].type,))
    if (float(w.xpos), float(w.ypos)) != (float(t.xpos), float(t.ypos)):
        raise NotImplementedError("VecRoket: p_wfss[0] looks at (%g, %g), p_targets[0] at (%g, %g): tomography needs "
                                  "a projector in the WFS direction, which does not exist here"
                                  % (w.xpos, w.ypos, t.xpos, t.ypos))
    return sup


class VecRoket(object):
    """The reference's error breakdown (guardians/roket_generalized_rl.py, RlErrorBudgetTester) for all environments
    of a VecAoEnv(..., geo=True, frame_pipeline=False).

    do_error_breakdown(action) sits where the reference's does: behind rl_step(apply_control=False,
    compute_tar_psf=False), before linear_step.  Nothing of the loop's state is touched: E, F and ageom are
    -cmat . slopes of slopes formed on scratch states that share the screens and read the mirrors' shapes.
      derr   -cmat . (the loop's slopes)
      E      noise-free sensor: derr itself; noisy: -cmat . (slopes of a second, noise-free formation, as
             denoiser.record_pairs forms it)
      F      -cmat . slopes_geom(atmosphere + mirrors in the WFS direction)
      ageom  -cmat . slopes_geom(that phase + the mirrors shaped by the geometric controller's fit of it): the part of
             the residual phase the mirrors cannot make (:235-247)
      B      the twin's command of this frame (next_part_one_geo ran behind the loop's do_control); fitting is its
             target's phase variance (twin.strehl[:, 2])
      G      None: the WFS and the target look the same way, tomography is identically zero.
    accumulate_from: first frame whose modal moments count (0: the reference's cov_cor, which includes the preloop;
    n_preloop is the documented alternative).  keep_envs: environments whose whole histories are kept on the host
    for save()."""

    def __init__(self, env, n_total, n_preloop, policy=None, gamma=1.0, accumulate_from=0, keep_envs=(),
                 psf_ortho_envs=()):
        import torch
        if n_total < n_preloop:
            raise ValueError("n_total (%d) < n_preloop (%d)" % (n_total, n_preloop))
        self.sup = sup = _roket_supervisor(env)
        self.env, self.policy = env, policy
        self.n_total, self.n_preloop, self.accumulate_from = int(n_total), int(n_preloop), int(accumulate_from)
        self.gamma = float(gamma)
        sim, s, cal = sup.sim, sup.s, sup.cal
        self.sim, self.nenv, self.device = sim, sim.nenv, sim.device
        self.nactu, self.nslope, self.nmodes = s.nactu, s.nslope, sup.nmodes
        self.nfiltered = max(int(sup.n_reverse_filtered_from_cmat), 0)
        self.delay = int(float(s.delay)) + 1
        self.g = float(sup.gain)
        self.cmat_h = np.ascontiguousarray(s.cmat, dtype=np.float32)
        self.RD = (self.cmat_h.astype(np.float64) @ np.asarray(cal.imat, dtype=np.float64)).astype(np.float32)
        self.bank = RoketBank(self.nenv, self.RD, cal.P, cal.Btt, self.g, self.gamma, self.nfiltered, self.delay,
                              ld_actu=sim.ld_actu, device=self.device)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.cmat = torch.as_tensor(self.cmat_h, device=self.device)                       # [nactu][nslope]
        self.Btt = torch.as_tensor(np.ascontiguousarray(cal.Btt, dtype=np.float32), device=self.device)
        n, ld = self.nenv, sim.ld_actu
        self.derr, self.E, self.F, self.ageom, self.rl_com = (torch.zeros(n, ld, **f32) for _ in range(5))
        self.rl_modes = torch.zeros(n, self.nmodes, **f32)
        self._ar = torch.as_tensor(np.asarray(sup.obtain_action_range_modal()) % self.nmodes, dtype=torch.long,
                                   device=self.device)
        self.noisy = float(s.noise) >= 0.0
        self.rad2_per_um2 = (2.0 * np.pi / float(s.tar_lambda)) ** 2       # phase variance, microns^2 -> rad^2 at the target
        # scratch states.  sc: the loop's screens and mirrors (shared, read only), everything written is its own.
        # sd: sc's sensor phase, its own mirrors -- shaped by the geometric fit of the residual phase.
        lib = sim.lib
        self.t = t = {}
        for k in ("com", "com1", "com2", "err"):
            t[k] = torch.zeros(n, ld, **f32)
        t["slopes"] = torch.zeros(n, s.nslope, **f32)
        t["wfs_phase"] = torch.zeros(n, s.n, s.n, **f32)
        t["tar_phase"] = torch.zeros(n, s.pupdiam, s.pupdiam, **f32)
        t["strehl"] = torch.zeros(n, 8, **f32)
        t["le_img"] = torch.zeros(n, (2 * s.strehl_halfwin) ** 2, **f32)
        t["frame"] = torch.zeros(n, dtype=torch.int32, device=self.device)
        t["work"] = torch.zeros(int(lib.aomarl_workspace_floats(sim.ctx, n)), **f32)
        t["gwork"] = torch.zeros(int(lib.aomarl_geo_workspace_floats(sim.ctx, n)), **f32)
        t["dm_shape"] = torch.zeros(n, sim.shape_stride, **f32)
        t["voltage"] = torch.zeros(n, ld, **f32)
        t["work2"] = torch.zeros_like(t["work"])
        sc = la.State()
        sc.nenv, sc.ld_actu = n, ld
        for k in ("screens", "origin", "seeds", "ext_count", "dm_shape", "voltage"):
            setattr(sc, k, sim.t[k].data_ptr())
        for k in ("com", "com1", "com2", "err", "slopes", "wfs_phase", "tar_phase", "strehl", "le_img", "frame", "work"):
            setattr(sc, k, t[k].data_ptr())
        sd = la.State()
        sd.nenv, sd.ld_actu = n, ld
        for k in ("screens", "origin", "seeds", "ext_count"):
            setattr(sd, k, sim.t[k].data_ptr())
        for k in ("com", "com1", "com2", "err", "slopes", "wfs_phase", "tar_phase", "strehl", "le_img", "frame",
                  "dm_shape", "voltage"):
            setattr(sd, k, t[k].data_ptr())
        sd.work = t["work2"].data_ptr()
        self.sc, self.sd = sc, sd
        self.keep_envs = [int(e) for e in keep_envs]
        self.psf_ortho_envs = [int(e) for e in psf_ortho_envs]
        for e in self.keep_envs + self.psf_ortho_envs:
            if not 0 <= e < n:
                raise ValueError("keep_envs / psf_ortho_envs: environment %d of %d" % (e, n))
        self.reset()

    # -------------------------------------------------------------------------------------------- bookkeeping
    def reset(self):
        import torch
        self.bank.reset()
        self.iter_number = 0
        z = lambda: torch.zeros(self.nenv, dtype=torch.float64, device=self.device)   # noqa: E731
        self._fit_sum, self._cg_sum, self._cg2_sum, self._n_behind = z(), z(), z(), 0
        self.psf_ortho = None
        self.hist = {k: [] for k in ("x", "com", "slopes", "wf_com", "alias_meas", "trunc_meas")}
        self.SR = self.SR2 = None

    def _neg_cmat(self, slopes, out):
        """out[:, :nactu] = -cmat . slopes on the library's fp32 GEMM (rtc.get_err: -CMAT.slopes)"""
        la.check(self.sim.lib.aomarl_gemm_nt(self.nenv, self.nactu, self.nslope, -1.0, slopes.data_ptr(),
                                             slopes.stride(0), self.cmat.data_ptr(), self.cmat.stride(0), 0.0,
                                             out.data_ptr(), out.stride(0), la.raw_stream(self.device)))
        return out

    @staticmethod
    def _centroid_gain(E, F):
        """rtc_util.centroid_gain of one frame: the slope of the straight line fitted to F against E"""
        Em = E - E.mean(dim=1, keepdim=True)
        Fm = F - F.mean(dim=1, keepdim=True)
        den = (Em * Em).sum(dim=1)
        return torch_where_pos(den, (Em * Fm).sum(dim=1) / den.clamp(min=1e-30))

    # -------------------------------------------------------------------------------------------- one frame
    def do_error_breakdown(self, action=None):
        """roket_generalized_rl.py:171-187 + error_breakdown (:286-376) for every environment."""
        import torch
        sup, sim, lib, ctx = self.sup, self.sim, self.sim.lib, self.sim.ctx
        sm, n, na = la.raw_stream(self.device), self.nenv, self.nactu
        sc, sd = C.byref(self.sc), C.byref(self.sd)
        with torch.no_grad():
            if sup._control_pending:
                raise RuntimeError("VecRoket: a do_control is pending (residual_shortcut): the breakdown reads the "
                                   "plain call order's state")
            # zeta's input: Btt . (rl * freedom) (:173-181)
            rl = None
            if self.policy is not None:
                if action is None:
                    raise ValueError("do_error_breakdown: a policy is set, action is required")
                a = torch.as_tensor(action, dtype=torch.float32, device=self.device)
                std = sup.config_rl["normalization_std_inside_environment"]
                mean = sup.config_rl["normalization_mean_inside_environment"]
                if std != 1.0 or mean != 0.0:
                    a = a * std + mean
                fv = torch.as_tensor(sup.freedom_vector, device=self.device)
                self.rl_modes.zero_()
                self.rl_modes[:, self._ar] = a * fv[self._ar]
                la.check(lib.aomarl_gemm_nt(n, na, self.nmodes, 1.0, self.rl_modes.data_ptr(), self.nmodes,
                                            self.Btt.data_ptr(), self.Btt.stride(0), 0.0, self.rl_com.data_ptr(),
                                            self.rl_com.stride(0), sm))
                rl = self.rl_com
            # the mirrors as the frame saw them, in memory (a pure function of the voltages)
            sim._set_defer(False)
            derr = self._neg_cmat(sim.t["slopes"], self.derr)
            # E: the noise-free sensor (:194-220)
            if self.noisy:
                la.check(lib.aomarl_comp_image(ctx, sc, 0, n, la.IMG_COG, sm))
                E = self._neg_cmat(self.t["slopes"], self.E)
                e_meas = self.t["slopes"].clone() if self.keep_envs else None
            else:
                E, e_meas = derr, (sim.t["slopes"] if self.keep_envs else None)
            # F: phase-derived slopes of the same phase (:222-233)
            la.check(lib.aomarl_raytrace_wfs(ctx, sc, 0, n, la.TRACE_ATMOS | la.TRACE_DMS | la.TRACE_RESET, sm))
            la.check(lib.aomarl_slopes_geom(ctx, sc, 0, n, sm))
            F = self._neg_cmat(self.t["slopes"], self.F)
            if self.keep_envs:
                self.hist["trunc_meas"].append((e_meas - self.t["slopes"])[self.keep_envs].cpu().numpy())
            # ageom: the geometric controller on the residual phase, its mirrors added to it (:235-247)
            la.check(lib.aomarl_raytrace_target(ctx, sc, 0, n, la.TRACE_ATMOS | la.TRACE_DMS | la.TRACE_RESET |
                                                la.TRACE_MASK, sm))
            la.check(lib.aomarl_geo_control(ctx, sc, 0, n, self.t["gwork"].data_ptr(), sm))
            fit = self.t["com"][:, :na].contiguous()
            la.check(lib.aomarl_comp_dm_shape(ctx, sd, 0, n, fit.data_ptr(), sm))
            la.check(lib.aomarl_raytrace_wfs(ctx, sd, 0, n, la.TRACE_DMS, sm))
            la.check(lib.aomarl_slopes_geom(ctx, sc, 0, n, sm))
            ageom = self._neg_cmat(self.t["slopes"], self.ageom)
            if self.keep_envs:
                self.hist["alias_meas"].append(self.t["slopes"][self.keep_envs].cpu().numpy())
            # B and the fitting term: the twin's frame (:341-348, 249-256)
            B = sup.geo.t["com"]
            if self.psf_ortho_envs and self.iter_number >= self.n_preloop:
                img = torch.stack([sup.geo.target_image(e, 1)[0] for e in self.psf_ortho_envs])
                self.psf_ortho = img if self.psf_ortho is None else self.psf_ortho + img
            # rtc.apply_control(0); comp_tar_image; comp_strehl (:184-186): what rl_step(apply_control=False,
            # compute_tar_psf=False) left out, by the supervisor's own call (it commits the twin's Strehl too, :253)
            sup.next_part_two(None, linear_control=True, apply_control=True, compute_tar_psf=True)
            if self.iter_number >= self.n_preloop:
                self._fit_sum += sup.geo.t["strehl"][:, 2].double()
                self._cg_sum += self._centroid_gain(E[:, :na], F[:, :na]).double()
                self._cg2_sum += self._centroid_gain(derr[:, :na], F[:, :na]).double()
                self._n_behind += 1
            self.bank.step(derr, E, F, ageom, B, None, rl, accumulate=self.iter_number >= self.accumulate_from)
            if self.keep_envs:
                x, b = self.bank.history()
                self.hist["x"].append(x[:, self.keep_envs].cpu().numpy())
                self.hist["wf_com"].append(b[3][self.keep_envs].cpu().numpy())     # G = B: wf_com is mod_com
                self.hist["com"].append(sim.com[self.keep_envs].cpu().numpy())
                self.hist["slopes"].append(sim.t["slopes"][self.keep_envs].cpu().numpy())
            self.iter_number += 1

    # -------------------------------------------------------------------------------------------- the run
    def run(self, verbose=True):
        """RlErrorBudgetTester.test_rl_agent_performance (error_budget_multiple_agents.py:284-343)."""
        import torch
        env, sup = self.env, self.sup
        self.reset()
        s = env.reset()
        linear = self.policy is None
        zero = torch.zeros(self.nenv, env.action_dim, device=self.device)
        if verbose:
            print("-----------------------------------------------------------------")
            print("iter# | SE SR | LE SR  (mean over %d environments)" % self.nenv)
            print("-----------------------------------------------------------------")
        for step in range(self.n_total):
            a = zero if linear else self.policy.select_action(s, eval_mode=True)[0]
            env.rl_step(a, linear_control=linear, apply_control=False, compute_tar_psf=False)
            self.do_error_breakdown(None if linear else a)
            s = env.linear_step()
            if verbose and (step + 1) % 100 == 0:
                sr = sup.get_strehl(0)
                print("%d \t %.4f \t  %.4f\t" % (step + 1, float(sr[:, 0].mean()), float(sr[:, 1].mean())))
            if step + 1 == self.n_preloop:
                sup.sim.reset_strehl()
        srs = sup.get_strehl(0)
        self.SR = srs[:, 1].double().cpu().numpy()
        # the reference's exp(srs[3]) is Marechal's estimate from the mean phase variance; here that variance is kept
        # in microns^2 (the phase's unit), hence the factor
        self.SR2 = np.exp(-srs[:, 3].double().cpu().numpy() * self.rad2_per_um2)
        return self.results()

    # -------------------------------------------------------------------------------------------- results
    def results(self):
        """Per environment (variances in microns^2: the Btt modes have unit geometric variance; x rad2_per_um2 for
        rad^2 at the target's wavelength): cov, cor (7x7 with a policy, 6x6 without; cov_cor, :441-480), the per-mode variance of
        every contributor and of their sum with and without zeta, the same summed over each agent's modes, fitting,
        SR, SR2, centroid_gain, centroid_gain2."""
        S1, S2, frames = self.bank.moments()
        with_zeta = self.policy is not None
        nb = max(self._n_behind, 1)
        out = dict(frames=frames, rad2_per_um2=self.rad2_per_um2, contributors=CONTRIBUTORS[:NC if with_zeta else NC - 1],
                   fitting=(self._fit_sum / nb).cpu().numpy(), SR=self.SR, SR2=self.SR2,
                   centroid_gain=(self._cg_sum / nb).cpu().numpy(), centroid_gain2=(self._cg2_sum / nb).cpu().numpy())
        cov, cor, var_k, var_sum, var_sum_nz = [], [], [], [], []
        for e in range(self.nenv):
            c, r, v = cov_cor_moments(S1[e], S2[e], frames, with_zeta)
            cov.append(c)
            cor.append(r)
            var_k.append(np.stack([v[k, k] for k in range(v.shape[0])]))
            var_sum.append(v.sum(axis=(0, 1)))                         # variance of the sum: every pair counts
            var_sum_nz.append(v[:NC - 1, :NC - 1].sum(axis=(0, 1)))
        out.update(cov=np.stack(cov), cor=np.stack(cor), var_modes=np.stack(var_k), var_modes_sum=np.stack(var_sum),
                   var_modes_sum_without_zeta=np.stack(var_sum_nz))
        layout = getattr(self.env, "layout", None)
        if layout is not None:
            rng = list(layout.agents.values())
            out["agent_ranges"] = rng
            out["var_agents"] = np.stack([out["var_modes"][:, :, a:b].sum(axis=2) for a, b in rng], axis=2)
            out["var_agents_sum"] = np.stack([out["var_modes_sum"][:, a:b].sum(axis=1) for a, b in rng], axis=1)
            out["var_agents_sum_without_zeta"] = np.stack(
                    [out["var_modes_sum_without_zeta"][:, a:b].sum(axis=1) for a, b in rng], axis=1)
        return out

    def save(self, path, envs=None):
        """An .npz per call with the reference's key names (save_in_hdf5, :402-436), histories [nactu][frames behind
        the preloop] with a leading axis over `envs` (a subset of keep_envs; default: all of them)."""
        d = self.to_dict(envs)
        np.savez(path, **d)
        return sorted(d)

    def to_dict(self, envs=None):
        """What save() writes, as a dictionary (psf_rec reads either)."""
        envs = list(self.keep_envs if envs is None else envs)
        if not envs or any(e not in self.keep_envs for e in envs):
            raise ValueError("save: envs=%r: histories were kept for keep_envs=%r only" % (envs, self.keep_envs))
        idx = [self.keep_envs.index(e) for e in envs]
        return npz_dict(self.hist, idx, envs, self.n_preloop, self.results(), self.sup.cal, self.cmat_h,
                        None if self.psf_ortho is None else (self.psf_ortho / max(self._n_behind, 1)).cpu().numpy(),
                        spup=self.sup.s.spupil, tar_lambda=self.sup.s.tar_lambda, psf_ortho_envs=self.psf_ortho_envs,
                        **self.groot_keys())

    def groot_keys(self):
        """What the GROOT model reads beside the matrices (groot.py): the stack array's coupling matrix and actuator
        positions, and the parameters under the reference's attribute names, as they stand now (set_wind / set_r0)."""
        from . import modal
        sup = self.sup
        ps, dm = sup.config, sup.s.dms[0]
        if dm.type != "pzt":
            raise NotImplementedError("VecRoket: the first mirror of the controller is %r, not a stack array" % (dm.type,))
        a, w, cz = ps.p_atmos, ps.p_wfss[0], np.cos(np.deg2rad(float(ps.p_geom.zenithangle)))
        frac = np.asarray(a.frac, dtype=np.float64)
        one = lambda v: np.asarray([v], dtype=np.float64)                  # noqa: E731
        params = {
            "_Param_atmos__r0": float(a.r0), "_Param_atmos__alt": np.asarray(a.alt, dtype=np.float64) / cz,
            "_Param_atmos__L0": np.asarray(a.L0, dtype=np.float64),
            "_Param_atmos__windspeed": np.asarray(a.windspeed, dtype=np.float64),
            "_Param_atmos__winddir": np.asarray(a.winddir, dtype=np.float64), "_Param_atmos__frac": frac / frac.sum(),
            "_Param_atmos__nscreens": int(a.nscreens), "_Param_loop__ittime": float(ps.p_loop.ittime),
            "_Param_controller__gain": float(sup.gain), "_Param_wfs__xpos": one(w.xpos), "_Param_wfs__ypos": one(w.ypos),
            "_Param_wfs__Lambda": one(w.Lambda), "_Param_wfs__nxsub": np.asarray([w.nxsub]), "_Param_wfs__npix": np.asarray([w.npix]),
            "_Param_wfs__noise": one(w.noise), "_Param_wfs__zerop": one(w.zerop), "_Param_wfs__gsmag": one(w.gsmag),
            "_Param_wfs__optthroughput": one(w.optthroughput), "_Param_wfs__pixsize": one(sup.s.cog_scale),
            "_Param_tel__diam": float(ps.p_tel.diam), "_Param_tel__cobs": float(ps.p_tel.cobs),
            "_Param_geom__pupdiam": int(sup.sysm.geom.pupdiam), "_Param_dm__nact": np.asarray([d.nact for d in ps.p_dms]),
            "_Param_dm__unitpervolt": np.asarray([d.unitpervolt for d in ps.p_dms], dtype=np.float64),
            # the sensor's own valid sub-apertures, in the order of its slopes (p_wfs._validsubsx, in pixels of the image)
            "_Param_wfs___validsubsx": np.asarray(sup.s.validsubsx), "_Param_wfs___validsubsy": np.asarray(sup.s.validsubsy)}
        return dict(nact=modal.nact_geom(dm.i1, dm.j1, dm.pitch, ps.p_dms[sup.s.dm_index[0]].coupling, dm.n2 - dm.n1 + 1),
                    dm_xpos=dm.xpos, dm_ypos=dm.ypos, params=params)


def npz_dict(hist, idx, envs, n_preloop, res, cal, cmat, psf_ortho=None, spup=None, tar_lambda=None, psf_ortho_envs=None,
             nact=None, dm_xpos=None, dm_ypos=None, params=None):
    """The dictionary save() writes.  hist: per-frame lists, "x" [7][kept][nactu] and "com", "slopes", "wf_com",
    "alias_meas", "trunc_meas" [kept][.]; idx: positions of `envs` among the kept environments.  spup (the reference's
    name, drax.get_pup) and tar_lambda (its attribute _Param_target__Lambda) are what the PSF reconstruction reads
    beside the histories (psf_rec.py); psfortho_envs: the environments psfortho's leading axis runs over.  nact ("Nact",
    tomo.create_nact_geom), dm_xpos / dm_ypos ("dm.xpos", "dm.ypos") and params (the reference's attributes, a mapping
    "_Param_<class>__<name>" -> value) are what the GROOT model reads (groot.py)."""
    x = np.stack(hist["x"])[n_preloop:]                                # [frames][7][kept][nactu]
    h = lambda k: np.stack(hist[k])[n_preloop:][:, idx].transpose(1, 2, 0)       # noqa: E731
    xk = lambda k: x[:, k][:, idx].transpose(1, 2, 0)                  # noqa: E731
    IF = cal.IF.tocsc()[:, :-2].T.tocsr().astype(np.float32)
    nan = np.asarray(np.nan)
    pick = lambda v: nan if v is None else np.asarray(v)[envs]         # noqa: E731
    d = {"noise": xk(0), "non linearity": xk(1), "aliasing": xk(2), "filtered modes": xk(3), "bandwidth": xk(4),
         "tomography": xk(5), "zeta_com": xk(6), "wf_com": h("wf_com"), "P": np.asarray(cal.P), "Btt": np.asarray(cal.Btt),
         "IF.data": IF.data, "IF.indices": IF.indices, "IF.indptr": IF.indptr,
         "TT": np.asarray(cal.IF.tocsc()[:, -2:].todense(), dtype=np.float32),
         "fitting": pick(res["fitting"]), "SR": pick(res["SR"]), "SR2": pick(res["SR2"]), "cov": pick(res["cov"]),
         "cor": pick(res["cor"]), "centroid_gain": pick(res["centroid_gain"]),
         "centroid_gain2": pick(res["centroid_gain2"]), "R": np.asarray(cmat, dtype=np.float32),
         "D": np.asarray(cal.imat, dtype=np.float32), "com": h("com"), "slopes": h("slopes"),
         "alias_meas": h("alias_meas"), "trunc_meas": h("trunc_meas"), "envs": np.asarray(envs)}
    if psf_ortho is not None:
        d["psfortho"] = psf_ortho
        if psf_ortho_envs is not None:
            d["psfortho_envs"] = np.asarray(psf_ortho_envs)
    if spup is not None:
        d["spup"] = np.asarray(spup, dtype=np.float32)
    if tar_lambda is not None:
        d["tar_lambda"] = np.asarray([tar_lambda], dtype=np.float64)
    if nact is not None:
        d["Nact"] = np.asarray(nact, dtype=np.float32)
    if dm_xpos is not None:
        d["dm.xpos"] = np.asarray(dm_xpos)
    if dm_ypos is not None:
        d["dm.ypos"] = np.asarray(dm_ypos)
    for k, v in (params or {}).items():
        if not k.startswith("_Param_"):
            raise ValueError("npz_dict: params key %r is not one of the reference's attribute names (_Param_...)" % (k,))
        d[k] = np.asarray(v)
    return d


def torch_where_pos(den, val):
    import torch
    return torch.where(den > 0, val, torch.zeros_like(val))
