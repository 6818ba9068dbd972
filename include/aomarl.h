/*
 * aomarl.h -- C ABI of the MI355X-native AO environment hot path (libaomarl_hip.so).
 *
 * DROP-IN BOUNDARY.  The reference (Tomeu7/AO-MARL) reaches its per-frame arithmetic through the
 * pybind11 modules `sutraWrap` / `carmaWrap` of COMPASS (shesha/sutra_wrap.py:4-38,46-72); there
 * is no C header in its tree.  Each entry point below names the native call it replaces and the
 * reference call site that drives it.  Differences by design:
 *   - every call is BATCHED over environments [env_begin, env_begin+env_count) (independent
 *     atmosphere seeds); batch size 1 reproduces the reference's single simulation;
 *   - state lives in caller-owned device buffers (aomarl_state): no hidden device<->host copies
 *     (the reference copies ~8 arrays per frame through np.array(d_xxx), rtcCompass.py:114,310);
 *   - every call takes an explicit hipStream_t and returns an int status (0 = ok); the message of
 *     the last failure on the calling thread is aomarl_last_error().
 * Plain C types only: pointers + sizes, no torch/HIP types in signatures (stream is void*).
 *
 * Conventions: fp32; flat pixel index p = x + n*y (x fast); per-env vectors are rows [env][i].
 */
#ifndef AOMARL_H
#define AOMARL_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AOMARL_MAX_LAYERS 8
#define AOMARL_MAX_DMS 4
#define AOMARL_ABI_VERSION 5

enum { AOMARL_DM_PZT = 0, AOMARL_DM_TT = 1 };

/* flags of aomarl_raytrace_* (sourceCompass.py:54-85: tel/atm/dms/reset arguments) */
enum { AOMARL_TRACE_ATMOS = 1, AOMARL_TRACE_DMS = 2, AOMARL_TRACE_RESET = 4,
       AOMARL_TRACE_MASK = 8 /* multiply the result by the pupil (geometric controller input) */ };
/* flags of aomarl_comp_image */
enum {
  AOMARL_IMG_FROM_PHASE_BUFFER = 1, /* read st->wfs_phase (else: fused integer-offset raytrace) */
  AOMARL_IMG_NOISE = 2,             /* apply photon / read-out noise if desc.noise >= 0       */
  AOMARL_IMG_WRITE_BINCUBE = 4,     /* store the 16x16 spot images (st->bincube)              */
  AOMARL_IMG_COG = 8,               /* fused centre of gravity -> st->slopes                  */
  AOMARL_IMG_NO_ATMOS = 16,         /* fused raytrace: DMs only (interaction matrix)          */
  AOMARL_IMG_NO_DMS = 32,           /* fused raytrace: atmosphere only                        */
  AOMARL_IMG_DM_FROM_VOLTAGE = 64   /* aomarl_frame_fused only: evaluate the stack-array DM phase
                                       from st->voltage on the fly (st->dm_shape's stack-array
                                       planes are not read; see aomarl_dm_from_voltage_available) */
};
/* bits of aomarl_apply_control's comp_voltage argument */
enum {
  AOMARL_APPLY_COMP_VOLTAGE = 1,     /* run the delay line (Rtc.apply_control's compVoltage)     */
  AOMARL_APPLY_DEFER_STACK_SHAPE = 2 /* do not materialise the stack-array shapes now: the next
                                        aomarl_frame_fused(DM_FROM_VOLTAGE) evaluates them from
                                        st->voltage; ignored when that path is unavailable.
                                        aomarl_materialize_dm_shape refreshes them on demand     */
};

typedef struct {
  int32_t type;          /* AOMARL_DM_PZT | AOMARL_DM_TT                                   */
  int32_t dim;           /* support is dim x dim (dm_init.py:146-147,168)                  */
  int32_t nact;
  int32_t influsize;     /* pzt: side of one influence patch (dm_init.py:373)              */
  int64_t ninflupos;     /* pzt: len(influpos)                                             */
  const float *influ;    /* pzt: [nact][ss][ss] = influ.flatten('F') of the (ss,ss,nact) cube
                            tt : [dim*dim][2]   = C-order (dim,dim,2) cube (dm_init.py:661-694) */
  const int32_t *influpos;   /* dm_init.py:800 */
  const int32_t *ninflu;     /* [dim*dim]  dm_init.py:804 */
  const int32_t *influstart; /* [dim*dim]  dm_init.py:805 */
  float wfs_xoff, wfs_yoff;  /* wfs_init.py:196-204  */
  float tar_xoff, tar_yoff;  /* target_init.py:119-141 */
} aomarl_dm_desc;

typedef struct {
  int32_t dim;          /* screen is dim x dim (atmos_init.py:94-96)              */
  int32_t nstencil;     /* iterkolmo.py:76-96                                      */
  const float *A;       /* [dim][nstencil] row-major (iterkolmo.py:229)            */
  const float *B;       /* [dim][dim]                (iterkolmo.py:239)            */
  const uint32_t *istx; /* [nstencil] flat logical indices, mirrored if deltax < 0 */
  const uint32_t *isty;
  float deltax, deltay; /* pixels per frame (atmos_init.py:99-102)                 */
  float amplitude;      /* r0_layer^(-5/6) * 0.5/(2 pi): screens in microns        */
  float wfs_xoff, wfs_yoff; /* wfs_init.py:177-185   */
  float tar_xoff, tar_yoff; /* target_init.py:104-113 */
} aomarl_layer_desc;

typedef struct {
  int32_t abi_version; /* = AOMARL_ABI_VERSION */
  /* pupil (geom_init.py:813-868) */
  int32_t n, pupdiam;
  const float *mpupil; /* [n*n]            */
  const float *spupil; /* [pupdiam*pupdiam] */
  /* Shack-Hartmann WFS (geom_init.py:168-321, 622-810; Sensors ctor wfs_init.py:107-110) */
  int32_t nvalid, pdiam, nfft, npix, nrebin, nxsub;
  const int32_t *phasemap; /* [pdiam^2][nvalid] */
  const float *halfxy;     /* [pdiam^2]         */
  const int32_t *binmap;   /* [nrebin^2][npix^2] */
  const float *flux;       /* [nvalid] fluxPerSub of valid subaps (wfs_init.py:145) */
  const int32_t *validsubsx, *validsubsy; /* [nvalid] pixel coords in binimg */
  float nphot, wfs_lambda, noise, cog_offset, cog_scale, subapd;
  /* atmosphere */
  int32_t nlayers;
  aomarl_layer_desc layers[AOMARL_MAX_LAYERS];
  /* DMs of the controller, stack arrays first, tip-tilt last */
  int32_t ndm;
  aomarl_dm_desc dms[AOMARL_MAX_DMS];
  /* science target */
  float tar_lambda;
  int32_t npsf;           /* FFT support of the PSF the window is cut from */
  int32_t strehl_halfwin; /* PSF evaluated on frequencies [-hw, hw) in x and y */
  /* controller (rtc_init.py:385-389, 506-513) */
  int32_t nactu, nslope;
  float gain, delay;
} aomarl_desc;

/* Device buffers owned by the caller (e.g. torch tensors); all [nenv] leading. */
typedef struct {
  int32_t nenv;
  int32_t ld_actu;     /* row stride (floats) of com/com1/com2/err/voltage, >= nactu, % 4 == 0 */
  float *screens;      /* [nenv][aomarl_screen_stride] ring-buffered phase screens (microns);
                          private layout, use aomarl_get_screen / aomarl_set_screen            */
  int32_t *origin;     /* [nenv][nlayers][2]     ring origin (ox, oy)                       */
  uint32_t *seeds;     /* [nenv]                 atmosphere base seed (layer k uses seed+k) */
  uint32_t *ext_count; /* [nenv][nlayers]        extrusions drawn so far (RNG counter)      */
  float *com, *com1, *com2, *err, *voltage; /* [nenv][nactu]                               */
  float *slopes;       /* [nenv][nslope]         all x then all y (ao_env.py:665-666)       */
  float *dm_shape;     /* [nenv][aomarl_dmshape_stride]: dim^2 per stack array, 4 per tip-tilt */
  float *bincube;      /* [nenv][nvalid][npix^2] or NULL                                    */
  float *wfs_phase;    /* [nenv][n*n]            or NULL (only the unfused API needs it)    */
  float *tar_phase;    /* [nenv][pupdiam^2]      or NULL                                    */
  float *strehl;       /* [nenv][8]: se, le, phase_var, phase_var_sum, count, peak_on_edge  */
  float *le_img;       /* [nenv][(2hw)^2]        long-exposure PSF window                   */
  uint32_t *frame;     /* [nenv]                 WFS noise frame counter                    */
  float *work;         /* aomarl_workspace_floats(ctx, nenv) floats                         */
} aomarl_state;

typedef struct aomarl_ctx aomarl_ctx;

const char *aomarl_last_error(void);
int aomarl_abi_version(void);

/* Arithmetic of the library (process-wide).  The reference computes in fp32 throughout (Rtc_FFF,
 * shesha/sutra_wrap.py:49; np.float32 arrays, shesha/init/wfs_init.py:76-101), and AOMARL_PRECISION_F32 --
 * fp32 operands on fp32 matrix instructions, fp32 vector arithmetic in every kernel -- is the default.
 * AOMARL_PRECISION_SPLIT_F16 is the opt-in fast mode: operands carried as fp16 pairs (hi + lo, 22-bit
 * mantissa, fp32 accumulation) in the three kernel families that have such a form: the DFTs of the
 * one-pass frame kernel, the internal GEMMs (extrusion, command matrix, Btt projections; see
 * aomarl_gemm_nt_split) and the denoiser (aomarl_denoiser_apply).  The per-family switches of
 * aomarl_set_option ("force_f32_dft", "gemm_split_f16") override it for one family.
 * aomarl_arith_*: launches per arithmetic family since aomarl_arith_reset, e.g.
 * "gemm:split_f16_mfma" -- bench.py builds its `dtype` from what was actually launched. */
enum { AOMARL_PRECISION_F32 = 0, AOMARL_PRECISION_SPLIT_F16 = 1 };
int aomarl_set_precision(int mode);
int aomarl_get_precision(void);
/* Fast mode only: number of kernel threads of split-fp16 GEMM launches on the current device since the
 * last query that staged an operand whose scaled value left the fp16 range (|v| > 65504: it is clipped
 * there, the product is wrong).  Synchronises `stream`, clears the counter.  The internal call sites keep
 * margins of 10^2 .. 10^4 over what a closed loop produces (stencil differences up to 255 um, Btt
 * coordinates up to 4094, slopes up to 65504 arcsec); a diverging policy can leave them.  ao_marl_amd.env
 * checks it at every episode boundary, like aomarl_denoiser_overflow.  ONE counter per device for the whole
 * process, cleared by whoever reads it first: with several contexts alive (training + evaluation) a clipping
 * event is reported to the first reader, whichever context it happened in. */
int aomarl_gemm_saturated(unsigned *count, void *stream);
int aomarl_arith_families(void);
const char *aomarl_arith_family_name(int family);
unsigned long long aomarl_arith_launches(int family);
void aomarl_arith_reset(void);

/* Build the static device-side description (replaces the Telescope/Atmos/Sensors/Dms/Target/
 * Rtc constructors + load_arrays calls of shesha/init/xxx_init.py). Host pointers are copied. */
int aomarl_create(const aomarl_desc *desc, aomarl_ctx **out);
int aomarl_destroy(aomarl_ctx *ctx);
/* d_control[0].set_cmat (basis.py:254): cmat is [nactu][nslope] row-major, host memory */
int aomarl_set_cmat(aomarl_ctx *ctx, const float *cmat);
int aomarl_set_gain(aomarl_ctx *ctx, float gain); /* d_control[0].set_gain (ao_env.py:957) */
/* One integrator gain per environment (host [nenv], nenv = st->nenv of the states stepped with this
 * context) instead of the scalar: the gain scan of obtain_best_gain_and_modes_filtered.py:101-150 as
 * ONE batch, environment e running the reference's loop with gain gains[e].  NULL: scalar again.
 * Applies to aomarl_do_control only; the RL control entry points take their gain as an argument. */
int aomarl_set_env_gains(aomarl_ctx *ctx, const float *gains, int nenv);
/* Per-mode integrator gains in Btt coordinates (upstream's modal optimisation, rtc_init.py:506-513: com -= gain *
 * mgain (.) err).  With e = -s2m . slopes (aomarl_slopes2modes) and m = v2m . com the law becomes
 *     m[t] = m[t-1] + gain * mgain[m] * e[t],   com[t] = m2v . m[t]
 * mgain: HOST [nrows][nmodes], a FACTOR on the scalar gain, copied; nrows == 1: one vector for all environments,
 * nrows == st->nenv: one per environment (checked where a state is at hand).  nmodes must equal the modal basis's
 * (aomarl_set_modal first).  Entries must be finite and >= 0.  NULL: cleared, every entry point issues the launches it
 * issued before.  All ones is the scalar law.  While gains are set:
 *   aomarl_do_control        err = -cmat . slopes as ever (unscaled: states and rewards read it), then
 *                            com += m2v . ((gain or the environment's gain of aomarl_set_env_gains) * mgain (.) e);
 *                            needs aomarl_set_slopes2modes
 *   aomarl_rl_control_modes  modes = m0 + (g * mgain[m]) * m1, in that order: with ones the bits of the scalar law
 *   aomarl_env_step / aomarl_policy_env_step   the general chain (aomarl_rl_control_modes, aomarl_apply_control, ...,
 *                            aomarl_do_control call by call): no fused head, small chain, residual shortcut, graph replay
 *                            or frame pipeline.  A context with a pipelined frame in flight refuses the call. */
int aomarl_set_modal_gains(aomarl_ctx *ctx, const float *mgain, int nrows, int nmodes);
/* The gains as set: mgain_out HOST [nrows][nmodes] or NULL (sizes only); nrows_out = 0 when none are set. */
int aomarl_get_modal_gains(aomarl_ctx *ctx, float *mgain_out, int *nrows_out, int *nmodes_out);
/* volts2modes [nmodes][nactu], modes2volts [nactu][nmodes] (rlSupervisor.py:170-172),
 * freedom vector [nmodes] (rlSupervisor.py:277-278), action_modes[nact]: the modes an action
 * component drives (rlSupervisor.py:677-691); host memory */
int aomarl_set_modal(aomarl_ctx *ctx, int nmodes, const float *v2m, const float *m2v,
                     const float *freedom, int nact, const int32_t *action_modes);
size_t aomarl_workspace_floats(const aomarl_ctx *ctx, int nenv);
size_t aomarl_screen_stride(const aomarl_ctx *ctx);   /* floats per env in st->screens  */
size_t aomarl_dmshape_stride(const aomarl_ctx *ctx);  /* floats per env in st->dm_shape */

/* RlSupervisor.reset (rlSupervisor.py:236-246): Atmos.set_seed/refresh_screen per layer
 * (atmosCompass.py:137-145), integrator + DM shapes + Strehl meter zeroed.
 * seeds: host [env_count]; accumx/accumy: host [nenv][nlayers], zeroed for the reset envs. */
int aomarl_reset(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                 const uint32_t *seeds, float *accumx, float *accumy, void *stream);

/* The next episode's reset, hidden behind the running one.  The trainer knows the next seeds while an episode
 * runs (train_rpc.py:486-487: `seed += 1`), and refresh_screen is 2 x dim DEPENDENT extrusions per layer
 * (atmosCompass.py:137-145) -- most of a reset's time.  aomarl_reset_prefetch_begin starts them in a SHADOW state
 * (own screens / origin / seeds / ext_count / frame / com, com1, com2, err, voltage / work; the other buffers may
 * alias the live state's: they are not touched), aomarl_reset_prefetch_advance runs `nrounds` more rounds (< 0: all
 * that are left) -- both on a stream of the caller's choice, beside the live episode --, and aomarl_reset_adopt is
 * aomarl_reset with the screens COPIED from the shadow (it first runs whatever rounds are left, on
 * prefetch_stream).  Same kernels on the same columns with the k split aomarl_reset's partition of the batch gives
 * its products ("reset_prefetch_whole" below): the screens are the plain reset's, bit for bit (tests/test_gpu_glue.py).  The seeds must be those of the begin call.
 * `*remaining` = rounds still to run.  aomarl_reset_prefetch_cancel forgets a begun prefetch. */
int aomarl_reset_prefetch_begin(aomarl_ctx *ctx, const aomarl_state *shadow, int env_begin, int env_count,
                                const uint32_t *seeds, void *stream);
int aomarl_reset_prefetch_advance(aomarl_ctx *ctx, int nrounds, void *stream, int *remaining);
int aomarl_reset_prefetch_cancel(aomarl_ctx *ctx);
int aomarl_reset_adopt(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count, const uint32_t *seeds,
                       float *accumx, float *accumy, void *prefetch_stream, void *stream);
/* Atmos.move_atmos (atmosCompass.py:161). accumx/accumy: host [nenv][nlayers], updated. */
int aomarl_move_atmos(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                      float *accumx, float *accumy, void *stream);
/* The same move, issued EARLY: call it after the last kernel of this frame that reads the screens
 * has been enqueued on `stream`; the extrusions run on a stream of the library behind that point,
 * beside whatever `stream` does next (do_control, the agents, next_part_two).  The next
 * aomarl_move_atmos of the same state / range only waits for it (the move is not repeated); every
 * other entry point that touches the screens waits for it too, aomarl_reset drops it.  Between the
 * two calls the screens are one frame ahead of the slopes.  The composite aomarl_next_part_one does
 * this by itself under aomarl_set_option(ctx, "prefetch_atmos", 1); not for states that share their
 * screens (the GEO twin).  Results are those of the plain call order, bit for bit. */
int aomarl_prefetch_atmos(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                          float *accumx, float *accumy, void *stream);
/* Run-time changes of the atmosphere (AtmosCompass.set_wind / set_r0, atmosCompass.py:79-135; the trainer's
 * non-stationary experiments, train_rpc.py:429-450).  Host values of the context: every move PLANNED after the call
 * uses them; a move already issued by aomarl_prefetch_atmos keeps the wind it was planned with (the host side
 * refuses to step across that: ao_marl_amd/env.py VecAtmos), a prefetched reset in flight must be cancelled by the
 * caller when a sign of deltax changes (its rounds run along the old sign).  Both calls synchronise the device.
 *
 * aomarl_set_wind = Tscreen.set_deltax + set_deltay of layer `layer` (pixels per frame), and -- the rule of
 * atmosCompass.py:124-135 -- where old * new < 0 along an axis that axis' stencil is mirrored
 * (istencil -> dim * dim - 1 - istencil: set_istencilx / set_istencily).  mirror_stencils = 0: the deltas alone
 * (the facade's set_deltax / set_deltay; it mirrors through aomarl_set_stencil).
 * aomarl_set_stencil = Tscreen.set_istencilx (axis 0) / set_istencily (axis 1): n = the layer's stencil size, flat
 * logical indices, host memory.
 * aomarl_set_r0 = Atmos.set_r0: the amplitude of the noise term of every layer's new lines, amplitude[nlayers] =
 * r0_layer^(-5/6) * 0.5 / (2 pi) in um (atmos_init.py:115, iterkolmo.py:278); the screens as they stand are kept. */
int aomarl_set_wind(aomarl_ctx *ctx, int layer, float deltax, float deltay, int mirror_stencils);
int aomarl_set_stencil(aomarl_ctx *ctx, int layer, int axis, const uint32_t *istencil, int n);
int aomarl_set_r0(aomarl_ctx *ctx, const float *amplitude, int nlayers);
/* the layer's current host values (deltax, deltay, amplitude); any pointer may be null */
int aomarl_get_layer(const aomarl_ctx *ctx, int layer, float *deltax, float *deltay, float *amplitude);
/* one parallel round of extrusions: op i extrudes layer[i] in direction dir[i] (+-1 x, +-2 y) */
int aomarl_extrude(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count, int nops,
                   const int32_t *layer, const int32_t *dir, void *stream);
/* overwrite one layer with logical screens src [env_count][dim*dim] (device); ring origin -> 0 */
int aomarl_set_screen(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count, int layer,
                      const float *src, void *stream);
/* copy the logical (un-rotated) screen of one layer to dst [env_count][dim*dim] (device) */
int aomarl_get_screen(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count, int layer,
                      float *dst, void *stream);

/* Source.raytrace for the WFS guide star / the target (sourceCompass.py:76-85), materialising
 * st->wfs_phase / st->tar_phase. The fast path (aomarl_comp_image without FROM_PHASE_BUFFER,
 * aomarl_target_psf) fuses this and never writes the phase. */
int aomarl_raytrace_wfs(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                        int flags, void *stream);
int aomarl_raytrace_target(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                           int flags, void *stream);
/* Wfs.comp_image (wfsCompass.py:343) [+ Rtc.do_centroids when AOMARL_IMG_COG] */
int aomarl_comp_image(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count, int flags,
                      void *stream);
/* Rtc.do_centroids (rtcCompass.py:563) from st->bincube */
int aomarl_do_centroids(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                        void *stream);
/* Wfs.slopes_geom(0) from st->wfs_phase (imats.py:103) */
int aomarl_slopes_geom(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                       void *stream);
/* Rtc.do_control (rtcCompass.py:547): err = -cmat.s ; com += gain*err */
int aomarl_do_control(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                      void *stream);
/* d_control[0].set_com (rtcCompass.py:473): com_dev [env_count][nactu] device memory */
int aomarl_set_com(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                   const float *com_dev, void *stream);
/* RlSupervisor.rl_control -> correction_modal_basis (rlSupervisor.py:713-733, 784-818):
 * m = v2m.com ; m[action_modes] += action*freedom[action_modes] ; com = m2v.m
 * action_dev [env_count][nact] device memory */
int aomarl_rl_control(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                      const float *action_dev, void *stream);
/* aomarl_rl_control when the Btt coordinates of the current command are already known:
 *     modes = m0 + g * m1 (+ action * freedom on the action modes) ; com = m2v . modes
 * (m0, m1, modes_out: device [env_count][nmodes], modes_out may be NULL; action may be NULL).
 * The commands never leave span(Btt) (cmat = Btt . D+, rl_control projects on it) and v2m . m2v = I,
 * so v2m . com of the command the integrator left, com_before + g * err, is v2m . com_before +
 * g * v2m . err by linearity -- two vectors the environment has just computed for its state
 * (AoEnv.linear_step, ao_env.py:871-909): the v2m GEMM of rl_control and the one of the next
 * state are saved.  ao_marl_amd/env.py uses it inside step(); results differ from aomarl_rl_control
 * by fp32 round-off only. */
int aomarl_rl_control_modes(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                            const float *m0_dev, const float *m1_dev, float g,
                            const float *action_dev, float *modes_out_dev, void *stream);
/* Rtc.apply_control (rtcCompass.py:582): delay line -> voltage -> Dm.comp_shape per DM;
 * comp_voltage: AOMARL_APPLY_* bits (1 = the reference's compVoltage=True) */
int aomarl_apply_control(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                         int comp_voltage, void *stream);
/* 1 when the one-pass frame kernel can evaluate the stack-array DM from the command lattice
 * (separable influence functions on a regular lattice whose pitch divides the 16-pixel tile) */
int aomarl_dm_from_voltage_available(aomarl_ctx *ctx);
/* Dm.comp_shape of every DM from st->voltage, also after AOMARL_APPLY_DEFER_STACK_SHAPE */
int aomarl_materialize_dm_shape(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                                void *stream);
/* Dm.set_com + comp_shape (dmCompass.py:64-146): volts_dev [env_count][nactu] or NULL=voltage */
int aomarl_comp_dm_shape(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                         const float *volts_dev, void *stream);
/* materialise the shape of DM k into dst [env_count][dim*dim] (device memory). Stack-array shapes
 * live in st->dm_shape; tip-tilt shapes are never stored (consumers evaluate c0*f0 + c1*f1) */
int aomarl_get_dm_shape(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count, int k,
                        float *dst, void *stream);
/* implementation switches for tests / A-B measurements: "force_generic_dm" (per-pixel gather
 * tables instead of the separable-lattice kernel), "force_valu_target" (VALU PSF rows kernel),
 * "force_generic_spot" / "force_generic_target" (layout-agnostic kernels), "force_unfused_frame"
 * (separate target and WFS passes in aomarl_next_part_one), "force_f32_dft" (one-pass frame
 * kernel: 1 = fp32 MFMAs through LDS tiles, 0 = split-fp16 MFMAs from registers, -1 = follow
 * aomarl_set_precision, the default), "precision" (= aomarl_set_precision; process-wide, ctx may be NULL),
 * "gemm_target_blocks" (split-K target of the fast mode's split-fp16 GEMM; the fp32 products run on k_gemm_p,
 * csrc/aomarl_gemm_p.h, which picks tile and k split so that every CU gets the same share),
 * "gemm_xcd_map" (default 1: the split-f16 GEMM's blocks are renumbered so that one XCD works on one k-chunk and
 * its L2 holds that slice of both operands; 0: plain grid order; same values; process-wide, ctx may be NULL),
 * "time_frame_kernel" (see aomarl_frame_kernel_time),
 * "gemm_split_f16" (1: the internal products on split-fp16 operands, see aomarl_gemm_nt_split; 0: on fp32
 * matrix instructions; follows aomarl_set_precision, i.e. 0, until set; process-wide),
 * "prefetch_atmos" (aomarl_next_part_one moves the next frame's atmosphere on a side stream, see
 * aomarl_prefetch_atmos),
 * "gemm_kgroups" (k-groups per tile of aomarl_gemm_batched: 0 = heuristic, 1 / 2 / 4; process-wide,
 * ctx may be NULL),
 * "reset_untransposed" (1: aomarl_reset runs its 2 n x-extrusions on the row-major screen itself; default 0:
 * on the transposed screen -- every new line a row instead of 648 scattered 4-byte writes -- followed by
 * one in-place transposition: same screens, bit for bit, 46 instead of 60 ms per 256 environments),
 * "extrude_unfused" (1: scatter and gather of two consecutive extrusion rounds with the same operations
 * as separate launches; default 0: one launch, k_extrude_sg -- same values),
 * "reset_streams" (default 2: a reset of >= 32 environments runs its 1296 dependent extrusion rounds in two
 * halves of the batch side by side, the second on the library's extrusion stream, each half's kernels filling the
 * other's latency -- 59 -> 51 ms per 256 environments; 1: one chain on the caller's stream; same kernels on the same
 * columns, the split-K rule of a product sees its half's columns; only with "prefetch_atmos" on),
 * "reset_prefetch_whole" (default 1: aomarl_reset_prefetch_* walks the rounds as ONE range whose products take the
 * tile and the k split a half's product gets -- a sum's order depends on the k split alone, so the screens are the
 * plain reset's bit for bit, with half the launches beside the running episode: 47 instead of 60 ms of rounds per 256
 * environments, the step beside them 2.7 % shorter; 0: the plain reset's halves one after the other),
 * "small_move" (default 1: screens of <= 256 pixels with stencil + dim <= 4096 -- the 10x10 files -- move in ONE
 * launch per frame, k_move_small, instead of gather / GEMM / scatter rounds; fp32 vector FMAs in both precision
 * modes; 0: the rounds),
 * "renew_frame_stream" (any value): the frame pipeline's own stream is destroyed and created anew -- the runtime deals
 *   its hardware queues out as streams come, and a frame stream that shares one with another stream of the step makes
 *   the pipelined order nearly twice as slow; nothing may be in flight (behind a full-range reset).  VecAoEnv's probe
 *   of the two call orders asks for it before it settles for the plain order.
 * "small_chain" (default 1: systems with <= 512 actuators / modes, <= 1024 slopes and nactu x nslope <= 65536 run the
 * control / agent chain of aomarl_env_step as two workgroup-per-environment kernels, k_small_head / k_small_tail,
 * instead of three GEMMs and five elementwise kernels; fp32 round-off apart, the same numbers; 0: the general chain),
 * "frame_pipeline" (default 1; 0 = plain call order although aomarl_set_frame_pipeline gave a twin; refused while
 * a frame is in flight),
 * "defer_dm_shape" (the composites
 * aomarl_next_part_two / aomarl_next_part_one use AOMARL_APPLY_DEFER_STACK_SHAPE /
 * AOMARL_IMG_DM_FROM_VOLTAGE when available: st->voltage is the DM state and the stack-array
 * planes of st->dm_shape stay stale until aomarl_materialize_dm_shape) */
int aomarl_set_option(aomarl_ctx *ctx, const char *name, int value);
/* fused target raytrace + PSF window + phase variance into a pending slot
 * (RlSupervisor.raytrace_target, rlSupervisor.py:845-855) */
int aomarl_target_psf(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                      void *stream);
/* aomarl_target_psf + aomarl_comp_image in ONE pass over the phase (the two halves of
 * RlSupervisor.next_part_one between move_atmos and do_control, rlSupervisor.py:829-843): the
 * sub-aperture tiles of the WFS are the 16 x 16 tiles of the pupil grid the target sees, so every
 * screen / DM pixel is read once and feeds both paths.  Needs the geometry to line up (WFS grid =
 * pupil grid + symmetric guard band, same integer offsets, binary pupil, DMs = [stack array,
 * tip-tilt]): aomarl_frame_fused_available() says whether it does
 * (and "force_unfused_frame" was not set).  flags as aomarl_comp_image minus FROM_PHASE_BUFFER /
 * NO_ATMOS / NO_DMS.  aomarl_next_part_one uses it automatically when available. */
int aomarl_frame_fused_available(aomarl_ctx *ctx);
/* Name of the kernel instantiation the last aomarl_frame_fused of this context launched, spelled
 * as rocprofv3 prints it ("k_frame_wave<3, 1, true, false, false, true>": layers, lattice blocks,
 * DM from voltage, noise, bincube, split-fp16 DFT); "" before the first launch.  bench.py matches
 * it against the kernel name recorded in the profiles/ file it takes the HBM traffic from. */
const char *aomarl_frame_kernel_name(aomarl_ctx *ctx);
/* Under aomarl_set_option(ctx, "time_frame_kernel", nlaunches) every k_frame_wave launch carries a HIP
 * event pair on its own stream, attached to the dispatch as its start / stop events
 * (hipExtLaunchKernelGGL: no marker packets of their own on the queue; the first `nlaunches` launches
 * after the option is set or the times were last read).  This reads them: sum of the launch durations and their count; waits for the
 * recorded launches, then starts over.  bench.py's roofline.achieved comes from here. */
int aomarl_frame_kernel_time(aomarl_ctx *ctx, double *total_ms, int *launches);
int aomarl_frame_fused(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count, int flags,
                       void *stream);
/* General batched fp32 GEMM (forward and backward passes of the stacked SAC networks):
 * C[b] = act(opA(A[b]) . opB(B[b]) + bias[b]) (+ C[b] if accumulate); opA(A) is M x K (stored [M][K],
 * or [K][M] when transA), opB(B) is K x N (stored [N][K], or [K][N] when transB).
 * y = x W, dx = dy W^T, dW = x^T dy of a layer with W stored [in][out] are (0,1), (0,0), (1,1). */
int aomarl_gemm_batched(int batch, int transA, int transB, int M, int N, int K, const float *A, int lda,
                        long long strideA, const float *B, int ldb, long long strideB, const float *bias,
                        long long strideBias, float *C, int ldc, long long strideC, int relu,
                        int accumulate, void *stream);
/* ---- multi-agent soft actor-critic update (the learner side of the path) --------
 * One call = update_critic -> update_actor -> update_alpha -> soft_update of EVERY agent on one
 * replay batch per agent (reference: SAC.update_critic / update_actor / update_alpha / soft_update,
 * src/reinforcement_learning/rpc_training/train_rpc.py:985-1038, 1044-1064, 1070-1084, 1128-1129,
 * networks src/reinforcement_learning/rpc_training/model_rpc.py:60-160), forward AND hand-derived
 * backward passes on the batched MFMA GEMM, Adam (torch.optim.Adam defaults) and the target update
 * fused into one kernel per parameter set.
 *
 * Parameters live in caller-owned flat device buffers (zero-padded per agent, fp32):
 *   policy : W1 [A][in_max][H], b1 [A][H], (Wh [A][H][H], bh [A][H]) x (n_hidden - 1),
 *            Whead [A][H][2 act_max] (mean | log_std columns), bhead [A][2 act_max]
 *   critic : Win [A][in_max + act_max][2 Hc] (Q1 | Q2 columns; rows: state then action),
 *            bin [A][2 Hc], Wout [A][2][Hc], bout [A][2]
 * each tensor starting on a multiple of 4 floats (aomarl_sac_layout returns the offsets). */
typedef struct {
  int32_t n_agents, batch, in_max, act_max, hidden, hidden_critic, n_hidden;
  int32_t state_dim, action_dim;         /* row lengths of the replay ring */
  const int32_t *state_gather;           /* host [A][in_max]: column of the state row, < 0 = zero pad */
  const int32_t *action_gather;          /* host [A][act_max]: column of the action row, < 0 = pad */
  const int32_t *n_act;                  /* host [A]: live action columns of each agent */
  const float *target_entropy;           /* host [A] */
  float gamma, tau, lr, beta1, beta2, adam_eps;
  float log_sig_min, log_sig_max, action_scale, action_bias;
  /* device buffers, caller-owned: parameters, Adam moments (m, v: zero before the first update) and
   * the gradients of the last update (written by every call, laid out like the parameters) */
  float *policy, *policy_m, *policy_v, *policy_grad;                  /* policy_len floats each */
  float *critic, *critic_m, *critic_v, *critic_grad, *critic_target;  /* critic_len floats each */
  float *log_alpha, *log_alpha_m, *log_alpha_v, *log_alpha_grad, *alpha;   /* [A] each */
} aomarl_sac_desc;
typedef struct aomarl_sac aomarl_sac;
#define AOMARL_SAC_SOFT_UPDATE 1      /* target <- (1 - tau) target + tau critic after the critic step */
#define AOMARL_SAC_TUNE_ALPHA 2       /* automatic entropy tuning */
/* offsets (floats) of the tensors inside the flat buffers; policy_off [2 n_hidden + 2] in the order
 * above, critic_off [4]; returns the two lengths. */
int aomarl_sac_layout(const aomarl_sac_desc *d, long long *policy_off, long long *critic_off,
                      long long *policy_len, long long *critic_len);
int aomarl_sac_create(const aomarl_sac_desc *d, aomarl_sac **out);
int aomarl_sac_destroy(aomarl_sac *s);
/* replay ring: state / next_state [rows][state_dim], action [rows][action_dim], reward [rows][A],
 * mask [rows].  idx: device [A][batch] row numbers (int64), or NULL: drawn uniformly in
 * [0, replay_rows) from Philox (seed, counter).  eps_next / eps_pi: device [A][batch][act_max]
 * standard-normal draws, or NULL: Philox (seed, counter).  adam_step: 1-based update count.
 * losses: device [5][A] (q1, q2, policy, alpha losses, alpha value) or NULL. */
int aomarl_sac_update(aomarl_sac *s, const float *state, const float *next_state, const float *action,
                      const float *reward, const float *mask, long long replay_rows, const int64_t *idx,
                      const float *eps_next, const float *eps_pi, uint32_t seed, uint32_t counter,
                      int adam_step, int flags, float *losses, void *stream);
/* ---- agent-side glue, all device pointers, no context (fused chains of the tiny host operations
 * the reference does per agent per step):
 * aomarl_split_states   TrainerRPC.divide_states_for_agents (train_rpc.py:418-427):
 *                       out[a][e][k] = state[e][gather[a][k]], gather == state_dim -> 0 (padding)
 * aomarl_policy_sample  GaussianPolicy.sample(only_choosing_action) on the head outputs
 *                       (model_rpc.py:137-144): head [A][nenv][2*act_max] = mean | log_std ->
 *                       action, mean [nenv][action_dim]; eps: standard normals [nenv][action_dim]
 *                       or NULL (Philox4x32-10 keyed by seed, counter = step, env, action index)
 * aomarl_assemble_state AoEnv.linear_step's concatenation + standardise (ao_env.py:470-480,
 *                       871-909): out[e] = concat_k (src_k[e] - mean_k) / std_k  (mean/std NULL:
 *                       raw); src / mean / std_ are HOST arrays of device pointers
 * aomarl_agent_rewards  helper_rewards.get_separated_rewards (helper_rewards.py:14-22):
 *                       out[e][a] = -factor * mean(res[e][lo_a:hi_a]^2), lohi [A][2] on the device */
int aomarl_split_states(int nenv, int state_dim, int n_agents, int in_max, const int32_t *gather,
                        const float *state, float *out, void *stream);
int aomarl_policy_sample(int nenv, int act_max, int action_dim, const float *head, float log_sig_min,
                         float log_sig_max, float scale, float bias, const int32_t *sc_agent,
                         const int32_t *sc_local, const float *eps, uint32_t seed, uint32_t counter,
                         float *action, float *mean, void *stream);
int aomarl_assemble_state(int nenv, int nblocks, const float *const *src, const int32_t *ld,
                          const int32_t *dim, const float *const *mean, const float *const *std_,
                          float *out, void *stream);
/* The same with a column selection: out block k = standardise(src_k[:, sel[0 .. dim_k)]) (the
 * action-range sub-selection of transform_state_to_zernike, ao_env.py:482-505). sel NULL = identity. */
int aomarl_assemble_state_cols(int nenv, int nblocks, const float *const *src, const int32_t *ld,
                          const int32_t *dim, const float *const *mean, const float *const *std_,
                          const int32_t *sel, float *out, void *stream);
int aomarl_agent_rewards(int nenv, int nmodes, int n_agents, const float *res_modes, int ld,
                         const int32_t *lohi, float factor, float *out, void *stream);
/* ---- one native call per half of a training step.  Same launches, same order as the entry points
 * above; what they save is the host: ~25 calls per step at ~10 us each from the Python side.
 *
 * aomarl_actor_forward   TrainerRPC.choose_action for every agent (train_rpc.py:650-675):
 *                        divide_states_for_agents -> GaussianPolicy.forward (Linear + ReLU stack, merged
 *                        mean | log_std head) -> sample(only_choosing_action) -> the global action vector.
 *                        Weights in nn.Linear layout, stacked over agents, zero-padded to in_max / act_max. */
typedef struct {
  int32_t n_agents, nenv, state_dim, in_max, act_max, hidden, n_hidden, action_dim;
  const int32_t *gather;               /* device [A][in_max]: state column, state_dim = zero pad      */
  const float *W1, *b1;                /* device [A][H][in_max], [A][H]                               */
  const float *const *Wh, *const *bh;  /* HOST arrays of n_hidden - 1 device pointers [A][H][H], [A][H] */
  const float *Whead, *bhead;          /* device [A][2 act_max][H], [A][2 act_max]                    */
  const int32_t *sc_agent, *sc_local;  /* device [action_dim]                                         */
  float log_sig_min, log_sig_max, scale, bias;
  float *x, *h0, *h1, *head;           /* device scratch [A][nenv][in_max], [A][nenv][H] x 2, [A][nenv][2 act_max]
                                          (only the layer-by-layer path uses them)                    */
  int32_t flags;                       /* AOMARL_ACTOR_*                                              */
  const float *W1_tiled;               /* device copies of W1 / Wh / Whead in the tile order of      */
  const float *const *Wh_tiled;        /* aomarl_actor_tile_weights (HOST array for Wh), or NULL      */
  const float *Whead_tiled;
} aomarl_actor_desc;
/* With the tiled copies at hand (and hidden % 16 == 0): ONE launch -- one workgroup per agent x 16
 * environments, activations in LDS, fp32 matrix instructions.  Without them, or with this flag:
 * split_states + one batched GEMM per layer + policy_sample.  Same arithmetic up to the order of the
 * fp32 sums. */
#define AOMARL_ACTOR_LAYER_BY_LAYER 1
/* dst[a] = the [N][K] matrix src[a] (nn.Linear layout, stacked over agents) cut into 16 x 16 tiles in
 * the operand order of the 16 x 16 x 4 matrix instruction, zero-padded: tile (n, s) holds 64 x float4,
 * entry l = row 16 n + (l & 15), columns 16 s + 4 (l >> 4) .. + 3.  dst: aomarl_actor_tiled_floats(). */
long long aomarl_actor_tiled_floats(int n_agents, int N, int K);
int aomarl_actor_tile_weights(int n_agents, int N, int K, const float *src, float *dst, void *stream);
int aomarl_actor_forward(const aomarl_actor_desc *d, const float *state, const float *eps, uint32_t seed,
                         uint32_t counter, float *action, float *mean, void *stream);
/* aomarl_env_step        TrainerRPC.env_step (train_rpc.py:633-648) for the default state layout
 *                        (dm_history_n .. 1, dm_before_linear, dm_residual; parameters.cfg:31-37), all
 *                        environments of the state:  rl_step (Btt correction through
 *                        aomarl_rl_control_modes, apply_control, Strehl)  ->  per-agent rewards  ->
 *                        linear_step (aomarl_next_part_one, v2m . err, standardise + concatenate).
 *                        The Btt coordinates of the last nhist + 1 commands live in a ring the caller
 *                        owns; ring_pos (slot of the newest) is advanced by the call. */
typedef struct {
  int32_t nmodes, dm_dim, n_agents, nhist;
  int32_t ring_pos;
  const int32_t *sel;                  /* device [dm_dim]: modes that enter the state, or NULL = all  */
  const float *mean_dm, *std_dm, *mean_res, *std_res;   /* device [dm_dim], or all NULL: raw states  */
  const int32_t *lohi;                 /* device [n_agents][2] mode ranges of the agents' rewards     */
  float reward_factor;
  float *modes_ring;                   /* device [nhist + 1][nenv][nmodes]                            */
  float *res_modes;                    /* device [nenv][nmodes]: v2m . err of the last frame (in/out) */
  void *denoiser;                      /* aomarl_denoiser* or NULL: the autoencoder branch of
                                          next_part_one_integrator (rlSupervisor.py:975-984); needs st->bincube */
  int32_t denoiser_f32;                /* 1: aomarl_denoiser_apply_f32                                 */
  int32_t flags;                       /* AOMARL_ENV_STEP_*                                            */
} aomarl_env_glue;
/* Default: the chain with every split-K reduction folded into the kernel that consumes the product and
 * independent small kernels sharing a launch (10 launches per step on the main stream).  With this
 * flag: the entry points above called one after the other (14).  Bit-identical results. */
#define AOMARL_ENV_STEP_UNFUSED 1
int aomarl_env_step(aomarl_ctx *ctx, aomarl_state *st, aomarl_env_glue *glue, const float *action_dev,
                    float gain, float *accumx, float *accumy, float *state_out, float *reward_out,
                    void *stream);
/* TrainerRPC.choose_action + TrainerRPC.env_step (train_rpc.py:650-675, 633-648) in ONE call: action = the actors on
 * `state` (aomarl_actor_forward's arguments), then aomarl_env_step with that action -> state_out (the next state),
 * reward_out: the two entry points one behind the other, from C -- one host round trip per step instead of two (a
 * host-bound step of a small system notices: BASELINE configs[1]).  action / mean: [nenv][action_dim] outputs. */
int aomarl_policy_env_step(aomarl_ctx *ctx, aomarl_state *st, aomarl_env_glue *glue, const aomarl_actor_desc *d,
                           const float *state_dev, const float *eps_dev, uint32_t seed, uint32_t counter, float gain,
                           float *accumx, float *accumy, float *action_dev, float *mean_dev, float *state_out,
                           float *reward_out, void *stream);
/* aomarl_set_option(ctx, "residual_shortcut", 1) (needs aomarl_set_slopes2modes): aomarl_env_step takes the residual
 * modes v2m . err of a frame from ONE product of its slopes with -(v2m . cmat) instead of aomarl_do_control (cmat . s,
 * integrate) + v2m . err: the integrator then lives in the Btt coordinates alone (the next call's head rebuilds the
 * command from them, as the reference's rl_control does every step: rlSupervisor.py:784-818), st->err is not formed and
 * st->com is not integrated in actuator space -- aomarl_do_control on the same slopes gives both afterwards.  Same
 * mathematics, another order of the fp32 sums (states within 3e-3 relative of the default's over 10 steps of the 40x40
 * system, tests/test_gpu_glue.py).  Returns 1 when a call with this glue would take the shortcut (the option is on, the
 * matrix matches the glue's modes, the chain is fusable and the system is not a small one, whose tail kernel does
 * do_control itself), else 0: a host that defers do_control must know (VecAoEnv._step_native). */
int aomarl_env_step_shortcut(aomarl_ctx *ctx, const aomarl_env_glue *glue);
/* Rtc.do_control (rtcCompass.py:547) for the whole batch on the slopes of the frame the last aomarl_env_step REDUCED:
 * with a frame in flight (aomarl_set_frame_pipeline) those live in the state or in its twin by parity, and the call-by-
 * call aomarl_do_control is refused; this one picks the view itself (err and com are not parity buffers, the next
 * call's head rebuilds com from the Btt coordinates before the delay line takes it).  Without a frame in flight:
 * aomarl_do_control of the whole batch.  What a host that runs with "residual_shortcut" calls when somebody asks for
 * err / the integrated command in actuator space (rtc.get_err / rtc.get_command, rtcCompass.py:114-142). */
int aomarl_do_control_reduced(aomarl_ctx *ctx, aomarl_state *st, void *stream);
/* aomarl_set_option(ctx, "graph_step", 1): aomarl_env_step replays a HIP graph captured from its own launch
 * sequence (one per distinct extrusion plan x ring position x buffer addresses; captured the first time a
 * combination occurs): one hipGraphLaunch instead of ~25 launches + ~8 event operations per step, for the
 * launch-bound regime (small batches).  Same kernels, same arguments, same results.  Inside a graph the side
 * streams join the caller's stream at the end of the step, so at large batches the plain path (whose
 * extrusion chain runs on beside the next step's head) is the faster one: off by default.
 * aomarl_graph_stats: graphs captured / replayed so far on this context. */
int aomarl_graph_stats(aomarl_ctx *ctx, unsigned long long *captures, unsigned long long *replays);

/* Frames one step ahead of the control chain ("frame pipeline").  With a loop delay of exactly one frame
 * (p_controller.delay == 1, the production files) the voltages frame t+1 is formed with are the commands
 * of step t (rlSupervisor.py next_part_two: the delay line of shesha's generic controller), known BEFORE
 * frame t's slopes have been reduced: the frame kernel of step t+1 does not depend on the control / agent
 * chain of step t.  aomarl_set_frame_pipeline hands the library a TWIN of `st` -- same aomarl_state, own
 * slopes / voltage / dm_shape / work buffers, every other pointer equal to st's -- and aomarl_env_step then
 * keeps one frame in flight: the call of step t launches frame t+1 on a stream of its own (even frames in
 * st's buffers, odd ones in the twin's; ring origins from per-parity snapshots), moves the atmosphere for
 * frame t+2 beside it when the lines that move rewrites lie outside the windows the frame kernel reads
 * (checked per move; otherwise behind it), and only then reduces frame t's slopes.  Same kernels, same
 * arguments, same values as the plain call order, bit for bit; the frame kernels run back to back with the
 * two latency chains beside them instead of between them.
 * Used only when the step is eligible (delay == 1, noise-free sensor, one-pass frame kernel with the DM
 * evaluated from the voltages, prefetch_atmos on, no denoiser, no graph_step, the whole batch); otherwise
 * aomarl_env_step takes the plain path.  While a frame is in flight the only calls accepted on this state
 * are aomarl_env_step and a full-range aomarl_reset (which drops it: the episode is over) -- everything
 * else fails loudly, because slopes / voltage of odd frames live in the twin and the screens are a frame
 * ahead.  twin == NULL switches the pipeline off (refused while a frame is in flight).
 * aomarl_frame_pipeline_state: in_flight = a frame is in flight; consumed_in_twin = the slopes / voltage of
 * the LAST REDUCED frame are in the twin's buffers; steps = pipelined steps so far; overlapped = moves that
 * ran beside the frame kernel. */
int aomarl_set_frame_pipeline(aomarl_ctx *ctx, const aomarl_state *st, const aomarl_state *twin);
int aomarl_frame_pipeline_state(aomarl_ctx *ctx, int *in_flight, int *consumed_in_twin,
                                unsigned long long *steps, unsigned long long *overlapped);

/* WFS-image denoiser in the loop (RlSupervisor.autoencoder_denoising, rlSupervisor.py:876-891;
 * DenoisingAutoencoderCNN2DSingleSubapeture.forward, src/autoencoder/autoencoder_models.py:130-197):
 * every 16 x 16 spot image of a bincube goes through the conv autoencoder, in place, in one fused
 * kernel.  weights / biases: 6 HOST arrays each in the reference checkpoint's layouts (encoder1..3
 * Conv2d [Cout][Cin][3][3]; decoder1, 2 ConvTranspose2d [Cin][Cout][4][4]; decoder3
 * ConvTranspose2d [16][1][3][3]).  cube: device [nimg][256], tiles [y][x] as aomarl_comp_image
 * writes them (the network sees them transposed, like the reference feeds them). */
typedef struct aomarl_denoiser aomarl_denoiser;
int aomarl_denoiser_create(const float *const *weights, const float *const *biases,
                           aomarl_denoiser **out);
/* In the library's precision mode (aomarl_set_precision): fp32 by default. */
int aomarl_denoiser_apply(aomarl_denoiser *dn, float *cube, long long nimg, void *stream);
/* Every product on fp32 matrix instructions (the reference's arithmetic; 4x the matrix-pipe time of the
 * split form). */
int aomarl_denoiser_apply_f32(aomarl_denoiser *dn, float *cube, long long nimg, void *stream);
/* Fast mode: each operand carried as an fp16 pair (hi + lo, 22 mantissa bits, fp32 accumulation): same
 * results to fp32 rounding as long as inputs and activations stay inside the fp16 range (|v| < 65504);
 * what leaves it is counted (aomarl_denoiser_overflow). */
int aomarl_denoiser_apply_split_f16(aomarl_denoiser *dn, float *cube, long long nimg, void *stream);
/* Number of kernel threads of split-fp16 denoiser launches since the last query that saw an activation
 * outside the fp16 range (the split-fp16 operands saturate there instead of overflowing loudly);
 * synchronises `stream`, clears the counter.  Non-zero: those results are wrong -- rerun on
 * aomarl_denoiser_apply_f32.  ao_marl_amd.denoiser checks it at every episode boundary. */
int aomarl_denoiser_overflow(aomarl_denoiser *dn, unsigned *count, void *stream);
int aomarl_denoiser_destroy(aomarl_denoiser *dn);
/* Training of the WFS-image denoiser (the module: src/autoencoder/autoencoder_models.py:130-197; the pairs it is
 * trained on: src/autoencoder/obtain_dataset_autoencoder.py:66-109.  The reference ships no training loop: the
 * loss, the mean squared error, and the optimiser, torch.optim.Adam's formula, are this library's choice).
 * weights / biases: 6 HOST arrays each in the checkpoint's layouts, as aomarl_denoiser_create takes them; any other
 * layer shape cannot be expressed.  lr, beta1, beta2, eps: torch.optim.Adam's (no weight decay; doubles, as torch
 * holds them; eps > 0).  max_batch sizes the workspace (about 300 KB per image, capped at 2048 images); larger batches are processed in passes of that size, their gradients added in a fixed order.
 * All products on fp32 matrix instructions; every sum over images and positions in a fixed order (no
 * floating-point atomics): the same inputs give the same bits. */
typedef struct aomarl_denoiser_trainer aomarl_denoiser_trainer;
int aomarl_denoiser_trainer_create(const float *const *weights, const float *const *biases, double lr,
                                   double beta1, double beta2, double eps, int max_batch,
                                   aomarl_denoiser_trainer **out);
int aomarl_denoiser_trainer_destroy(aomarl_denoiser_trainer *tr);
/* One optimisation step on `nimg` pairs: forward (autoencoder_models.py:176-197, sigmoid branch off), loss =
 * mean((net(noisy) - clean)^2) over nimg * 256 pixels, backward, Adam with bias correction.  noisy, clean:
 * device [nimg][256], tiles [y][x] (the network sees them transposed, as in aomarl_denoiser_apply).
 * loss_out: device float (the loss BEFORE the update) or NULL.  Asynchronous on `stream`. */
int aomarl_denoiser_trainer_step(aomarl_denoiser_trainer *tr, const float *noisy, const float *clean,
                                 long long nimg, float *loss_out, void *stream);
/* The same gradients without the update.  grads_w / grads_b: 6 DEVICE arrays each in the checkpoint's layouts
 * (an entry may be NULL). */
int aomarl_denoiser_trainer_grads(aomarl_denoiser_trainer *tr, const float *noisy, const float *clean,
                                  long long nimg, float *const *grads_w, float *const *grads_b,
                                  float *loss_out, void *stream);
/* The current weights into 6 + 6 DEVICE arrays in the checkpoint's layouts (what aomarl_denoiser_create and
 * SubapDenoiser take, once on the host). */
int aomarl_denoiser_trainer_get(aomarl_denoiser_trainer *tr, float *const *weights, float *const *biases,
                                void *stream);
/* ROKET error breakdown (guardians/roket_generalized_rl.py:189-284, 441-480): the loop filters of the seven
 * contributors {noise, trunc (non linearity), alias, H_com (filtered modes), bp (bandwidth), tomo, zeta} and the modal
 * moments of their covariance table, for nenv environments at once.  The reference keeps [n_iter][nactu] histories on
 * the host; this object keeps the last `delay` frames on the device and sums the moments as it goes.
 * RD = cmat . imat [nactu][nactu], P [nmodes][nactu], Btt [nactu][nmodes]: HOST arrays, row-major, copied.
 * gRD = g * gamma * RD is formed inside (:161).  delay = int(p_controllers[0].delay) + 1 (:163), 1..64.
 * nfiltered: the modes [-nfiltered-2 : -2] are the filtered ones (:258-264). */
typedef struct {
  int32_t nenv, nactu, ld_actu, nmodes, nfiltered, delay;
  float g, gamma;
  const float *RD, *P, *Btt;
} aomarl_roket_desc;
typedef struct aomarl_roket aomarl_roket;
int aomarl_roket_create(const aomarl_roket_desc *desc, aomarl_roket **out);
int aomarl_roket_destroy(aomarl_roket *r);
/* Frame t of the breakdown.  derr, E, F, ageom, B, G, rl_com: device [nenv][ld_actu], this frame's
 * -cmat.slopes of the loop (derr), of the noise-free image (E), of the geometric slopes (F), of the geometric slopes
 * of the DM-orthogonal phase (ageom), the geometric controller's commands in the target direction (B) and in the WFS
 * direction (G), and Btt . (the policy's modes) (rl_com).  G == NULL means G = B: tomography is identically zero and
 * its products are skipped.  rl_com == NULL: zeta stays zero.  Then
 *   noise_buf = derr - E, trunc_buf = E - gamma F, H_com / mod_com / wf_com from P, Btt and the filtered range,
 *   tomo_buf = mod_com - wf_com, and  x[t] = x[t-1] - gRD x[t-delay] + u[t-delay]  with u = g noise_buf,
 *   g trunc_buf, gamma g ageom, rl_com; bandwidth takes -(mod_com[t] - mod_com[t-1]) undelayed, tomography
 *   -g gamma RD tomo_buf[t-delay], as the reference does.  History before frame 0 is zero.
 * accumulate != 0: y_k = P x_k and, per environment and mode, S1[k] += y_k, S2[k <= l] += y_k y_l in double.
 * Every sum in a fixed order, no atomics: the same inputs give the same bits.  Asynchronous on `stream`. */
int aomarl_roket_step(aomarl_roket *r, const float *derr, const float *E, const float *F, const float *ageom,
                      const float *B, const float *G, const float *rl_com, int accumulate, void *stream);
/* S1_out: DEVICE double [nenv][7][nmodes]; S2_out: DEVICE double [nenv][28][nmodes], pairs (k, l), k <= l, k major;
 * frames_out: HOST, the number of accumulated frames.  Any may be NULL. */
int aomarl_roket_moments(aomarl_roket *r, double *S1_out, double *S2_out, long long *frames_out, void *stream);
/* zero histories, moments and the frame counter (synchronises the device) */
int aomarl_roket_reset(aomarl_roket *r);
/* x_out: DEVICE [7][nenv][nactu], the contributors of the last frame; bufs_out: DEVICE [4][nenv][nactu], its
 * noise_buf, trunc_buf, tomo_buf, mod_com.  Either may be NULL. */
int aomarl_roket_history(aomarl_roket *r, float *x_out, float *bufs_out, void *stream);
/* Modal gain optimisation (Gendron & Lena 1994; upstream's init_modalOpti / modalControlOptimization are not in the
 * reference tree): a bank of loop filters over recorded OPEN-loop residual modes x[t] = -s2m . slopes (mirrors flat).
 * For every environment, mode and candidate gain g_j it runs this simulator's loop for one mode,
 *     e[t] = x[t] - (wa c[t-1] + wb c[t-2] + wc c[t-3]),   c[t] = c[t-1] + g_j e[t]      (history before frame 0: zero)
 * with (wa, wb, wc) the delay-line weights of aomarl_apply_control, and sums J[env][mode][j] += e[t]^2 over t >= nskip.
 * State and sums are double on the device; one thread owns its (series, gains) for a whole call: no atomics, no
 * reduction across threads, the same inputs give the same bits, and a series fed in pieces gives the bits of one call.
 * gains: HOST [ngain], copied, any finite values; delay in [0, 2]. */
typedef struct {
  int32_t nenv, nmodes, ngain, nskip;
  float delay;
  const float *gains;
} aomarl_modopti_desc;
typedef struct aomarl_modopti aomarl_modopti;
int aomarl_modopti_create(const aomarl_modopti_desc *desc, aomarl_modopti **out);
int aomarl_modopti_destroy(aomarl_modopti *m);
/* zero filter states, sums and the frame counter (synchronises the device) */
int aomarl_modopti_reset(aomarl_modopti *m);
/* x_dev: DEVICE fp32, frame f of the chunk at x_dev + f * frame_stride, each an [nenv][nmodes] slab
 * (frame_stride >= nenv * nmodes).  Asynchronous on `stream`. */
int aomarl_modopti_accumulate(aomarl_modopti *m, const float *x_dev, int nframes, long long frame_stride, void *stream);
/* J_out: DEVICE double [nenv][nmodes][ngain].  argmin_out: DEVICE int32 [nenv][nmodes], the index of the smallest J among
 * the STABLE candidates (a non-finite J counts as +inf; ties, and so all-zero series, take the lowest gain; -1 when no
 * candidate is stable).  stable_out: HOST int32 [ngain], 1 where the cubic of that gain has all roots inside the unit
 * circle (g = 0, the open loop, counts as stable).  frames_out: HOST, frames accumulated so far.  Any may be NULL. */
int aomarl_modopti_result(aomarl_modopti *m, double *J_out, int32_t *argmin_out, int32_t *stable_out,
                          long long *frames_out, void *stream);
/* The same bank ON-LINE, in closed loop, on pseudo-open-loop modes (ao_marl_amd/modal_gains.py OnlineLoopBank is the
 * float64 statement).  x[t] = e[t] + p[t] with e[t] = -s2m . slopes[t] and p[t] = v2m . voltage[t], the voltage
 * aomarl_apply_control applied in the frame whose slopes these are: whatever produced it -- integrator, agents, any
 * delay -- x is the series the mirrors-flat loop would have measured, to the modal round trip.  Per frame and candidate
 *     e = x - (wa c0 + wb c1 + wc c2),  c <- (c0 + g e, c0, c1),  J = forget J + e^2 for frames whose index since the
 *     last restart is >= nskip
 * and every `period` frames (counted over all frames pushed, once a frame has entered J)
 *     j* = argmin over the stable candidates of J (pool = 0) or of sum_env J in ascending environment order (pool = 1),
 *     G <- G + beta (gains[j*] - G) in double,   mgain = float(G / gain) where a context is attached.
 * One [nenv][nmodes] row per frame goes into a device ring of `chunk` rows; the bank kernel consumes it when it is full
 * or an apply is due.  No host synchronisation, read-back or allocation per frame; no atomics; reruns, and chunk = 1
 * against chunk = 32, give the same bits.  G0: HOST double [rows][nmodes], rows = pool ? 1 : nenv; NULL: zeros. */
typedef struct {
  int32_t nenv, nmodes, ngain, nskip;
  int32_t chunk, period, pool;
  float delay;
  double forget, beta;
  const float *gains;
  const double *G0;
} aomarl_modopti_online_desc;
typedef struct aomarl_modopti_online aomarl_modopti_online;
int aomarl_modopti_online_create(const aomarl_modopti_online_desc *desc, aomarl_modopti_online **out);
/* refused while attached to a context (detach first) */
int aomarl_modopti_online_destroy(aomarl_modopti_online *m);
/* an episode reset: rows waiting in the ring are consumed, then c0..c2 and the since-restart counter are zeroed; J, G and
 * the apply schedule go on.  Asynchronous on `stream`. */
int aomarl_modopti_online_restart(aomarl_modopti_online *m, void *stream);
/* One frame: x_dev DEVICE fp32 [nenv][nmodes] (recorded telemetry, a caller's own reconstruction ...).  An apply that falls
 * due updates G (and the attached context's modal gains, if any).  Asynchronous on `stream`. */
int aomarl_modopti_online_push(aomarl_modopti_online *m, const float *x_dev, void *stream);
/* Rows waiting in the ring are consumed first.  J_out: DEVICE double [nenv][nmodes][ngain]; argmin_out: DEVICE int32
 * [rows][nmodes], the candidate the last apply chose (-1 before the first); G_out: DEVICE double [rows][nmodes];
 * stable_out: HOST int32 [ngain]; counts_out: HOST [4]: frames pushed, frames since the last restart, frames that entered
 * J, applies.  Any may be NULL. */
int aomarl_modopti_online_result(aomarl_modopti_online *m, double *J_out, int32_t *argmin_out, double *G_out,
                                 int32_t *stable_out, long long *counts_out, void *stream);
/* x_out: DEVICE fp32 [nenv][nmodes], the row pushed last (it stays in the ring after the bank has read it) */
int aomarl_modopti_online_last(aomarl_modopti_online *m, float *x_out, void *stream);
/* While attached, aomarl_do_control of the whole state `st` under modal gains forms p = v2m . st->voltage (one more
 * product), writes x = e + p into the ring between the s2m product and the gain scaling, and behind the command update
 * runs whatever the schedule asks for -- the bank, the apply that writes the context's DEVICE modal gains: gains derived
 * from frames <= t act from the do_control of frame t + 1.  A call with gain 0 (err alone, nothing integrated) is not a
 * frame of the loop and is not fed.  aomarl_get_modal_gains then returns the device's values (it
 * synchronises); aomarl_set_modal_gains is refused.  m = NULL detaches (the gains stay as last applied) and every entry
 * point issues the launches it issued before.  Refused: no modal gains set, or their row count not 1 (pool) / nenv (no
 * pool); per-environment scalar gains; a gain that is not positive; a pipelined frame in flight; nenv / nmodes that do
 * not match; and, while attached, aomarl_do_control on a partial environment range of `st`. */
int aomarl_modopti_online_attach(aomarl_ctx *ctx, aomarl_state *st, aomarl_modopti_online *m);
/* Modal PREDICTIVE control: one recursive-least-squares predictor per (environment, Btt mode) on the pseudo-open-loop
 * modes x[t] = e[t] + p[t] above (ao_marl_amd/predictive.py PredictorBank is the float64 statement;
 * csrc/aomarl_predictor_fn.h the update).  With h[s] = (x[s], ..., x[s-order+1]), zero before the last restart, and f the
 * frames since it:
 *     phi = wa h[t-1] + wb h[t-2] + wc h[t-3];   eps = x[t] - theta . phi
 *     f >= nskip:               J = forget J + eps^2,  J0 = forget J0 + x[t]^2
 *     learning, f >= order + 2: q = P phi, den = forget + phi . q, theta += q eps / den, P = (P - q q^T / den) / forget,
 *                               and P *= order p0 / trace(P) where the trace exceeds order p0
 *     c[t] = theta . h[t]       (theta after the update; rounded once to fp32)
 * from theta = (1, 0, ...), P = p0 I.  One lane per series, double throughout, the state in registers for all the frames
 * of a call; no atomics, no reduction: reruns and any split of the frames over calls give the same bits.  No host
 * synchronisation, read-back or allocation per frame. */
typedef struct {
  int32_t nenv, nmodes, order, nskip;      /* order 1..8 */
  float delay;                             /* 0..2, as aomarl_apply_control's */
  double forget, p0;                       /* forget in (0, 1]; p0 > 0, in units of 1 / x^2 */
} aomarl_predictor_desc;
typedef struct aomarl_predictor aomarl_predictor;
int aomarl_predictor_create(const aomarl_predictor_desc *desc, aomarl_predictor **out);
/* refused while attached to a context (detach first) */
int aomarl_predictor_destroy(aomarl_predictor *p);
/* an episode reset: the past values and the since-restart counter are zeroed; theta, P, J, J0 carry over.  Asynchronous. */
int aomarl_predictor_restart(aomarl_predictor *p, void *stream);
/* on != 0: theta and P are updated (the default); 0: frozen -- c, J and J0 go on */
int aomarl_predictor_set_learning(aomarl_predictor *p, int on);
/* nframes rows of recorded telemetry: x_dev DEVICE fp32, row t at x_dev + t * frame_stride, each [nenv][nmodes];
 * c_out_dev DEVICE fp32 [nframes][nenv][nmodes] or NULL.  One launch; the state is loaded once.  Refused while attached. */
int aomarl_predictor_push(aomarl_predictor *p, const float *x_dev, int nframes, long long frame_stride, float *c_out_dev,
                          void *stream);
/* theta_out: DEVICE double [nenv][nmodes][order]; P_out: DEVICE double [nenv][nmodes][order][order] (full, symmetric);
 * J_out, J0_out: DEVICE double [nenv][nmodes]; counts_out: HOST [3]: frames pushed, frames since the last restart, frames
 * that updated theta.  Any may be NULL. */
int aomarl_predictor_get(aomarl_predictor *p, double *theta_out, double *P_out, double *J_out, double *J0_out,
                         long long *counts_out, void *stream);
/* theta, P: HOST doubles in aomarl_predictor_get's layouts (checkpoints, warm starts); either may be NULL.  P must be
 * symmetric with a positive diagonal.  Synchronises. */
int aomarl_predictor_set(aomarl_predictor *p, const double *theta, const double *P);
/* x_out, c_out: DEVICE fp32 [nenv][nmodes]: the row consumed last and the command modes it gave.  Either may be NULL. */
int aomarl_predictor_last(aomarl_predictor *p, float *x_out, float *c_out, void *stream);
/* While attached, aomarl_do_control of the whole state `st` forms err as ever, e = -s2m . slopes, p = v2m . st->voltage and
 * x = e + p, runs the predictor on x (one launch) and sets com = m2v . c in place of the integration; and
 * aomarl_rl_control_modes composes modes = c (+ action * freedom on the action modes): m0, m1 and g are accepted and
 * ignored.  A call with gain 0 (err alone) is not a frame of the loop and is not fed.  p = NULL detaches, and every entry
 * point issues the launches it issued before.  Refused: no modal gains set (they route every step to the general
 * chain; their values are not used while attached, and aomarl_set_modal_gains(NULL) is refused); an on-line gain
 * optimiser attached (aomarl_modopti_online_attach refuses a context with a predictor likewise); per-environment
 * scalar gains; a pipelined frame in flight; nenv / nmodes that do not match; and, while attached, aomarl_do_control on
 * a partial environment range of `st`. */
int aomarl_predictor_attach(aomarl_ctx *ctx, aomarl_state *st, aomarl_predictor *p);
/* PSF reconstruction from the covariance of the ROKET error buffers, the Vii algorithm (guardians/gamora.py:24-100
 * psf_rec_Vii, :103-171 psf_rec_vii_cpu).  For the eigenpairs (e_k, V_k) of the modal covariance and the phase maps
 * m_k = IF^T (Btt V_k)[:-2] + TT (Btt V_k)[-2:] on the lit pixels of a p x p pupil, zero-padded to N x N (:148-159):
 *     tmp  = Re( fft2(sum_k e_k m_k^2) . conj(fft2 pup) ) - sum_k e_k |fft2 m_k|^2     (the first term is linear in m_k^2)
 *     dphi = Re ifft2(2 tmp) . den . mask . (2 pi / lambda)^2                             (:163)
 *     otf2 = exp(-dphi / 2) . mask / max                                                  (:164-165)
 *     psf  = fftshift Re ifft2(otf_other . otf2) . N^2 / npts                             (:167-168, :85-94)
 * The object keeps var = sum_k e_k m_k^2 on the lit pixels and acc = sum_k e_k |fft2 m_k|^2 on N/2 + 1 columns.
 * All HOST arrays of the desc are copied.
 *   p, N, npts          pupil side, transform size (a power of two, 32..2048, N >= 2 p), number of lit pixels
 *   lit [npts]          flat index y * p + x of the lit pixels, ascending: np.where(spup) order (:150)
 *   nactu, ld_actu      commands per vector (stack-array actuators, then tip and tilt) and the row stride of `com`
 *   if_data / if_indices / if_indptr   the file's CSR of the stack-array influence functions, [nactu - 2][npts]
 *                       (drax.get_IF); turned into a per-pixel tap list, at most 16 taps per pixel
 *   tt [npts][2]        the tip and tilt planes on the lit pixels
 *   denmask, mask, otftel [N][N]   den . mask . (2 pi / lambda)^2, mask, otftel / max: made in float64 by the caller
 *                       (:128-133; the mask is a threshold that fp32 transforms cannot reproduce at N = 2048) */
typedef struct {
  int32_t p, N, npts, nactu, ld_actu;
  const int32_t *lit;
  const float *if_data;
  const int32_t *if_indices, *if_indptr;
  const float *tt;
  const float *denmask, *mask, *otftel;
} aomarl_psfrec_desc;
typedef struct aomarl_psfrec aomarl_psfrec;
/* Allocates the whole workspace and transforms the pupil; nothing is allocated afterwards. */
int aomarl_psfrec_create(const aomarl_psfrec_desc *desc, aomarl_psfrec **out);
int aomarl_psfrec_destroy(aomarl_psfrec *r);
/* com: DEVICE [nk][ld_actu], the command vectors Btt V_k (:154); w: DEVICE [nk], their weights e_k (any sign).
 * For k = 0 .. nk-1 in order: m_k on the lit pixels, var += w_k m_k^2, acc += w_k |fft2 m_k|^2 (:155-159).  Every
 * element of var and acc is summed in k order by the thread that owns it, without atomics: one call of nk vectors and
 * several calls over the same vectors in the same order leave the same bits.  Asynchronous on `stream`. */
int aomarl_psfrec_accumulate(aomarl_psfrec *r, const float *com, const float *w, int nk, void *stream);
/* dphi, otf2, psf: DEVICE [N][N], any may be NULL (:163-168).  otf_other: DEVICE [N][N], the factor of the last
 * product -- the fitting OTF Re fft2(psfortho) / max (:85-90) -- or NULL for otftel / max (:92).  The accumulated
 * state is left as it is: a second call gives the same bits, and more vectors may be accumulated afterwards. */
int aomarl_psfrec_finish(aomarl_psfrec *r, const float *otf_other, float *dphi, float *otf2, float *psf, void *stream);
/* var = acc = 0 (synchronises the device) */
int aomarl_psfrec_reset(aomarl_psfrec *r);
/* GROOT: the residual-error covariance MODELLED from the atmosphere's structure functions (guardians/groot.py; the
 * structure functions: guardians/starlord.py:10-140).  The three covariances are one form over a point set p_i
 * (actuators, or sub-apertures):
 *     out[b][i][j] = sum_t w[b][t] F_kind(t)( |p_j - p_i + o[b][t]| ; x0, L0[b][t] )
 * with F = dphi_lowpass (Cerr, compute_Cerr_cpu :145-186), dphi_highpass (Calias, compute_Calias :590-599 with
 * compute_Calias_element_XX / _YY :633-700) or rodconan (dCmm, compute_dCmm_element :842-903).  F and the sum over the
 * taps are evaluated in double, in the taps' order; out is rounded to float once.
 *   n_max, batch_max    largest point set and most batch entries of one aomarl_groot_form call
 *   m_max, k_max        aomarl_groot_sandwich: most rows of G and largest order of C (both 0: no sandwich workspace)
 *   tabx, taby          HOST [10000]: the Ij0 table of starlord.tabulateIj0 (:56-72), x = e^t for t in [-4, 10]; copied */
typedef struct {
  int32_t n_max, batch_max, m_max, k_max;
  const double *tabx, *taby;
} aomarl_groot_desc;
#define AOMARL_GROOT_CERR 0
#define AOMARL_GROOT_CALIAS_XX 1
#define AOMARL_GROOT_CALIAS_YY 2
#define AOMARL_GROOT_DCMM_XX 3
#define AOMARL_GROOT_DCMM_YY 4
/* One model for `batch` atmospheres; all arrays HOST [batch][nlayers], read before the call returns.
 *   CERR       w = (1 / r0)^(5/3) frac (lambda_tar / 2 pi)^2 per layer, (sx, sy) = vdt u(theta) + Htheta u(angleht),
 *              vdt = speed ittime / gain (:152-170, :183-186), x0 = the actuator pitch (:160), L0 per layer
 *   CALIAS_*   nlayers = 1, w = 1/2 (1 / r0)^(5/3) c^2 (h / 3)^2 (:562-563, :609), x0 = d the sub-aperture size, npts
 *              the (odd) number of Simpson points (:612-630); sx, sy, L0 are not read
 *   DCMM_*     w = frac scale (:827, :837), (sx, sy) = ws dt u(wd) (:859-860), x0 = d, L0 per layer */
typedef struct {
  int32_t model, batch, nlayers, npts;
  double x0;
  const double *w, *sx, *sy, *L0;
} aomarl_groot_form_desc;
typedef struct aomarl_groot aomarl_groot;
/* Allocates the table, the tap buffers and the sandwich's workspace; no device or pinned memory is allocated afterwards
 * (a form call builds its tap list in a host vector). */
int aomarl_groot_create(const aomarl_groot_desc *desc, aomarl_groot **out);
int aomarl_groot_destroy(aomarl_groot *g);
/* px, py: DEVICE double [n], the points; out: DEVICE float, out[b * stride_o + i * ldo + j].  One thread owns one
 * element and adds its taps in order: entry b of a batched call and the same atmosphere alone leave the same bits.
 * Every w, sx, sy, L0 must be finite (refused by name otherwise).  Asynchronous on `stream`, except that a call first
 * waits for the object's previous form call to finish, on whatever stream that ran: the object has one tap buffer.  The
 * sandwich's workspace is not guarded in that way: use one stream per object for aomarl_groot_sandwich. */
int aomarl_groot_form(aomarl_groot *g, const aomarl_groot_form_desc *f, const double *px, const double *py, int n,
                      float *out, int ldo, long long stride_o, void *stream);
/* out [m][ldo] (+)= G [m][ldg] . C [n][ldc] . G^T in fp32 (the projections of :200-209, :601-606): two products on the
 * loop's fp32 matrix kernel, T = G C^T then out = G T^T; k splits are summed in a fixed order.  All DEVICE; G and C:
 * 16-byte aligned, ldg and ldc multiples of 4.  accumulate != 0 adds to out.  Asynchronous on `stream`. */
int aomarl_groot_sandwich(aomarl_groot *g, const float *G, int ldg, int m, const float *C, int ldc, int n, float *out,
                          int ldo, int accumulate, void *stream);
/* PSF window + phase variance of st->tar_phase as it stands (pending, like aomarl_target_psf) */
int aomarl_target_psf_buffer(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                             void *stream);
/* Target.get_tar_image(tar_index, expo_type = "se") (shesha/supervisor/components/targetCompass.py:71-92): the whole
 * short-exposure PSF of every environment of the range, out [env_count][npsf][npsf] ([ky][kx], zero frequency at
 * (npsf/2, npsf/2): what fftshift(np.array(d_image_se)) holds, transposed to this library's [y][x] order), raw
 * |FFT2|^2 like d_image_se.  On demand only -- the hot path forms the central window (aomarl_target_psf); three
 * reward branches of the reference read the full frame (ao_env.py:621-623, 654-656).  Two DFT passes on the
 * library's fp32 GEMM, one environment at a time; the phase is ray-traced from the state as it stands (stack-array
 * shapes are materialised first if they are deferred). */
int aomarl_target_image(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count, float *out, void *stream);
/* Geometric ("GEO") reference controller: COMPASS's sutra_controller_geo as the reference sets it
 * up (rtc_init.py:418-448 init_proj_sparse over the pupil pixels) and drives it
 * (rlSupervisor.py:989-1013: target.raytrace(atmosphere) -> rtc.do_control(sources=target) ->
 * apply_control -> target.raytrace(dms)).  The command is the least-squares projection of the
 * piston-removed pupil phase on the influence functions, tip-tilt first, stack array on the rest:
 *     com = W . [ IF_stack^T (m phi) | TT^T (m phi) | sum(m phi) ]
 * with W [nactu][nactu+1] (row-major, host) from ao_marl_amd.modal.geo_projector.  The products
 * are evaluated as two small batched GEMMs over the separable lattice + one GEMM against the
 * tip-tilt planes.  st->tar_phase must hold the MASKED atmosphere phase of the target
 * (aomarl_raytrace_target with ATMOS | RESET | MASK); the result goes to st->com.  A GEO twin is a
 * second aomarl_state that shares screens / origin / seeds / ext_count with the main one and owns
 * com / voltage / dm_shape / tar_phase / strehl / le_img / work.  `work`: device scratch of
 * aomarl_geo_workspace_floats(ctx, nenv) floats. */
int aomarl_set_geo(aomarl_ctx *ctx, const float *W);
size_t aomarl_geo_workspace_floats(aomarl_ctx *ctx, int nenv);
int aomarl_geo_control(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                       float *work, void *stream);
/* Target.comp_image + comp_strehl (targetCompass.py:193,205): publish the pending PSF */
int aomarl_comp_strehl(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                       void *stream);
/* Target.comp_strehl(do_fit = True), the default of the reference's get_strehl (targetCompass.py:139-159): the Strehl
 * record of an environment is 8 floats -- [0] SR SE, [1] SR LE, [2] phase variance, [3] its sum, [4] frames, [5] peak on
 * the window edge, [6] SR SE with the PSF peak fitted by two 1-D sincs (filled by every commit: the fit comes with
 * the window), [7] SR LE fitted -- which THIS call brings up to date from the accumulated window (it is not on the
 * control chain; between two calls slot 7 holds the un-fitted value of the last commit).  Reads only the state's
 * own record and long-exposure window: allowed while a pipelined frame is in flight. */
int aomarl_strehl_fit(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count, void *stream);
int aomarl_reset_strehl(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                        void *stream);
/* modes[row][nmodes] = v2m . vec[row][0..nactu)  (AoEnv.transform_state_to_zernike,
 * ao_env.py:482-505); vec_dev row stride ldvec >= nactu, modes_dev row stride nmodes; st may be
 * NULL (then no split-K workspace is used) */
int aomarl_volts2modes(aomarl_ctx *ctx, aomarl_state *st, int nrows, const float *vec_dev,
                       int ldvec, float *modes_dev, void *stream);
/* Residual in Btt coordinates straight from the slopes:  v2m . err = -(v2m . cmat) . slopes.  Where the
 * next control step takes its command from modal coordinates (aomarl_rl_control_modes) the frame
 * needs neither err nor the integrated com in actuator space, so ONE product with the pre-multiplied
 * matrix s2m = v2m . cmat (host, [nmodes][nslope]; NULL drops it) replaces aomarl_do_control +
 * aomarl_volts2modes; aomarl_do_control run later on the same slopes gives err / com exactly as the
 * plain order would.  AoEnv.linear_step's get_err -> transform_state_to_zernike (ao_env.py:507-533). */
int aomarl_set_slopes2modes(aomarl_ctx *ctx, int nmodes, const float *s2m);
int aomarl_slopes2modes(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count, float *modes,
                        void *stream);

/* composites: one call per half frame, same order as the reference
 * next_part_one: move_atmos, target trace(+PSF), WFS trace+image+COG, do_control
 *                (rlSupervisor.py:1015-1051, 954-987)
 * next_part_two: [rl_control], apply_control, comp_strehl (rlSupervisor.py:900-947);
 *                action_dev may be NULL (integrator only, linear_control=True) */
int aomarl_next_part_one(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                         float *accumx, float *accumy, int image_flags, void *stream);
int aomarl_next_part_two(aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count,
                         const float *action_dev, void *stream);

/* generic fp32 MFMA GEMM used by the calls above, exported for tests:
 * C[M][N] = alpha * A[M][K] . B[N][K]^T + beta * C ; device pointers, row-major, ld in floats; K >= 1 (an empty
 * sum is refused, here and in aomarl_gemm_nt_split) */
int aomarl_gemm_nt(int M, int N, int K, float alpha, const float *A, int lda, const float *B,
                   int ldb, float beta, float *C, int ldc, void *stream);

/* The same product on the f16 matrix pipe with split operands (hi + lo fp16 pairs, 22 mantissa bits,
 * fp32 accumulation; the kernel behind the library's own extrusion / command-matrix / Btt-projection
 * products unless aomarl_set_option(ctx, "gemm_split_f16", 0)): A and B are scaled by the powers of two
 * scale_a / scale_b as they are staged (undone in the result), the scaled magnitudes must stay below
 * 65504.  work (device, may be NULL): split-K workspace of work_floats floats.  Exported for tests. */
int aomarl_gemm_nt_split(int M, int N, int K, float alpha, const float *A, int lda, const float *B, int ldb,
                         float beta, float *C, int ldc, float scale_a, float scale_b, float *work,
                         long long work_floats, void *stream);

/* aomarl_gemm_nt as the loop's products call it -- with a split-K workspace, so that k_gemm_p writes partial slabs
 * work[z][M][N] and k_gemm_reduce sums them -- plus forcing and a report.  Exported for tests: the exact-arithmetic
 * conformance tests (tests/test_gpu_gemm_exact.py) run every kernel, tile instantiation and k split through it.
 * Forcing fields, 0 = the library's own choice (then the call goes through the per-shape memo like any other):
 *   kernel      1 = k_gemm_p, 2 = k_gemm_nt (also on 16-byte aligned operands), 3 = k_gemm_nt_h (scale_a / scale_b:
 *               powers of two as in aomarl_gemm_nt_split, 0 = 1)
 *   wm, wn      k_gemm_p's block tile (32 wm) x (32 wn); must be one of the instantiated tiles
 *   ksplit      k-chunks asked for (whole k-tiles per chunk: fewer may come out, see r_nz)
 *   xcd         1 = blocks renumbered by k-chunk per XCD, 2 = plain order, 0 = the "gemm_xcd_map" option
 *   pick_M      tile and k split as a product of pick_M rows would get them
 *   slabs_only  no reduce is launched and C is left untouched when the product was split: the caller sums
 *               r_slabs slabs work[z][M][N] and multiplies by r_alpha (r_slabs == 0: C is final)
 * Report: r_kernel (1 / 2 / 3), r_wm, r_wn (2, 2 for the 64 x 64 kernels), r_nz chunks of r_kchunk, and p_*: what
 * k_gemm_p's cost model picks for this shape and workspace, computed afresh (p_wm == 0: operands not aligned).
 * epi_mode   1: C = v, epi_com[m][n] += (epi_gain_row ? epi_gain_row[m] : epi_gain) * v  (the integrator);
 *            2: C = v + epi_action[m][j] * epi_freedom[n] where j = epi_amode_inv[n] >= 0  (the agents' action);
 *            applied by the reduce only when the product was split: r_fused says whether it was (else C = v alone,
 *            as for the library's own callers, who then run the step themselves).  Not with slabs_only.
 * A forced tile outside the menu, a forced kernel the operands' alignment rules out, or a forced split whose slabs
 * do not fit work_floats is an error that names the argument; nothing is launched and nothing is substituted.
 * No option is read for a forced field and none is set.  The per-shape memo of tile and k split is the library's own
 * path: it is read and written whenever both are left to the library (also when only kernel, xcd or pick_M is
 * forced), and neither read nor written when wm / wn or ksplit is forced. */
typedef struct aomarl_gemm_probe {
  int32_t kernel, wm, wn, ksplit, xcd, pick_M, slabs_only;
  float scale_a, scale_b;
  int32_t r_kernel, r_wm, r_wn, r_nz, r_kchunk, r_slabs;
  float r_alpha;
  int32_t p_wm, p_wn, p_nz, p_kchunk;
  /* the consumer's step folded into the split-K reduce (k_gemm_reduce_epi), epi_mode 0 = none: */
  int32_t epi_mode, epi_ldcom, epi_nact;
  float epi_gain;
  float *epi_com;
  const float *epi_gain_row, *epi_action;
  const int32_t *epi_amode_inv;
  const float *epi_freedom;
  int32_t r_fused;
} aomarl_gemm_probe;
int aomarl_gemm_nt_probe(int M, int N, int K, float alpha, const float *A, int lda, const float *B, int ldb,
                         float beta, float *C, int ldc, float *work, long long work_floats, aomarl_gemm_probe *probe,
                         void *stream);

/* The learner's grouped GEMM (k_gemm_g, csrc/aomarl_gemm_g.h) with everything its launch takes.  Exported for tests:
 *   C[g][M][N] = epilogue( opA(A[g]) . opB(B[g]) ),  g < groups
 *   ak: A is [M][K] (k contiguous), else [K][M];  bk: B is [N][K], else [K][N]
 *   epilogue: + bias[g][n] (may be NULL), ReLU (relu != 0), zero where mask[g][m][n] <= 0 (mask may be NULL);
 *   colsum (may be NULL; only with bk == 0): colsum[g][n] = sum_k B[g][k][n], written once
 *   force_wm, force_wn: block tile (32 wm) x (32 wn) with wm, wn in {2, 4}; 0 = the library's pick
 * Refused, as the kernel cannot take them: A or B not 16-byte aligned, lda / ldb / sA / sB not multiples of 4,
 * a leading dimension shorter than its row, colsum with bk != 0, a tile that is not instantiated.
 * Not restricted, because the kernel reads and writes them through 4-byte aligned accesses (16-byte pieces of C, bias
 * and mask are packed float quadruples, the ragged end of a row goes element by element): C, bias, mask and colsum at
 * any float address, any ldc / ldm >= N, any sC / sBias / sM / sCs (the tests run ldc = N + 3 and ldm = N + 1). */
typedef struct aomarl_gemm_g_args {
  int32_t groups, ak, bk, M, N, K;
  const float *A; int32_t lda; long long sA;
  const float *B; int32_t ldb; long long sB;
  float *C; int32_t ldc; long long sC;
  const float *bias; long long sBias;
  int32_t relu;
  const float *mask; int32_t ldm; long long sM;
  float *colsum; long long sCs;
  int32_t force_wm, force_wn;
} aomarl_gemm_g_args;
int aomarl_gemm_g_probe(const aomarl_gemm_g_args *args, void *stream);

/* batched fp32 MFMA GEMM with fused bias + ReLU for the stacked SAC MLPs (one batch entry per
 * agent): C[b][M][N] = act(A[b][M][K] . B[b][N][K]^T + bias[b][N]); B is in nn.Linear layout
 * ([out][in]); bias may be NULL; strides in floats; A, B 16-byte aligned */
int aomarl_gemm_nt_batched(int batch, int M, int N, int K, const float *A, int lda, long long strideA,
                           const float *B, int ldb, long long strideB, const float *bias,
                           long long strideBias, float *C, int ldc, long long strideC, int relu,
                           void *stream);

/* Pyramid wavefront sensor ("pyrhr": four pupil images, modulation, field stop) looking at a pupil phase such as
 * aomarl_raytrace_wfs leaves in st->wfs_phase.  The model is ao_marl_amd/pyramid.py:PyramidModel ("Pyramid
 * sensor"); the geometry comes from geometry.pyr_geometry (reference: geom_init.py:init_pyrhr_geom).  Per environment
 * and modulation point k:  f_k = mpupil exp(i (2 pi / lambda phi + cx_k (x - n/2) + cy_k (y - n/2))), centred in an
 * Nfft^2 zero array;  F_k = fft2(f_k) exp(i halfxy) submask;  hr += w_k |ifft2 F_k|^2, k in index order.  Then the
 * pixel filter (hr = Re ifft2(fft2(hr) sincar)), sums over nrebin x nrebin blocks, the flux scale
 * nphotons / (sum_k w_k  sum mpupil^2), optional noise (the draw rule of the Shack-Hartmann pixels, one Philox block per
 * (pixel, frame), idx = flat pixel index) and the slopes (all x, then all y).
 * Arrays of the desc are HOST arrays, copied by create.  validsubsx / validsubsy: [4 nvalid], ROW and COLUMN of the
 * pixel in the [Nfft / nrebin]^2 image, four blocks of nvalid in the reference's order (blocks at row-,col- / row+,col+
 * / row+,col- / row-,col+ of the centre).  x slope of point i: ((q1 + q3) - (q0 + q2)) / norm, y slope:
 * ((q1 + q2) - (q0 + q3)) / norm with q_j the pixel of block j. */
typedef struct {
  int32_t nenv, n, Nfft, nrebin, nvalid, npts_max, pixel_filter;
  int32_t batch_kib;  /* KiB the intermediate planes of a batch may occupy; 0: the default (inside the last-level cache) */
  float lambda_um;   /* wavelength of the sensor in microns (the phase is in microns) */
  float nphotons;    /* photons per frame over the whole aperture */
  float noise;       /* < 0: none; 0: photon noise; > 0: + read-out noise of that many electrons rms */
  float thresh;      /* a normaliser below it gives slope 0 */
  const float *mpupil;                     /* [n][n] */
  const float *halfxy, *submask, *sincar;  /* [Nfft][Nfft], zero frequency at index 0 */
  const int32_t *validsubsx, *validsubsy;  /* [4 nvalid] */
} aomarl_pyr_desc;
typedef struct aomarl_pyr aomarl_pyr;
enum { AOMARL_PYR_NOISE = 1 };
/* Allocates the whole workspace; nothing is allocated afterwards.  The modulation starts as one point on the tip
 * (cx = cy = 0, weight 1, s_scale 1) and the reference slopes as zero. */
int aomarl_pyr_create(const aomarl_pyr_desc *desc, aomarl_pyr **out);
int aomarl_pyr_destroy(aomarl_pyr *p);
/* cx, cy [rad / pixel of the pupil], w: HOST [npts], 1 <= npts <= npts_max; s_scale: the slopes' unit (arcsec).
 * Synchronises the device. */
int aomarl_pyr_set_modulation(aomarl_pyr *p, const float *cx, const float *cy, const float *w, int npts, float s_scale);
/* ref: HOST [2 nvalid], subtracted from every slope vector; NULL: zero.  Synchronises the device. */
int aomarl_pyr_set_ref(aomarl_pyr *p, const float *ref);
/* phase: DEVICE [nenv][n * n] microns; environments env_begin .. env_begin + env_count - 1 are measured.
 * image: DEVICE [nenv][(Nfft / nrebin)^2] or NULL; slopes: DEVICE [nenv][2 nvalid] or NULL (rows of the environments
 * measured are written).  method 0 .. 3 (0 / 1: normalised by the mean intensity over the valid points, 2 / 3: by the
 * point's own; 1 / 3: s_scale sin(pi / 2 raw), 0 / 2: s_scale raw).  flags & AOMARL_PYR_NOISE: the desc's noise is
 * drawn with seeds[e] and frame[e] (DEVICE [nenv], as aomarl_state has them) and frame[e] advances by one.
 * No atomics: every pixel is summed over the modulation points in index order by the thread that owns it, so the bits
 * do not depend on how the environments are split into calls.  Asynchronous on `stream`; no allocation, no read-back. */
int aomarl_pyr_measure(aomarl_pyr *p, const float *phase, int env_begin, int env_count, int flags, int method,
                       const uint32_t *seeds, uint32_t *frame, float *image, float *slopes, void *stream);

/* Mirror mis-registration per environment (reference: dmCompass.py:148-176, set_dm_registration(dm_index, dx, dy, theta,
 * G), which forwards dx / pixsize, dy / pixsize, theta and G to the native mirror).  A table [nenv][ndm][6] of fp32
 * numbers {A00, A01, A10, A11, tx, ty} on the device: pixel (x, y) of a source's grid (nn = n for the sensor, pupdiam for
 * the target; c = (nn - 1) / 2; (ox, oy) the mirror's offset on that grid) samples mirror k of environment e at
 *   (u, v) = (c + ox, c + oy) + A (x - c, y - c) + t
 * by the bilinear rule of aomarl_raytrace_wfs / _target, unchanged (floor cell outside [0, dim): 0; neighbour index
 * clamped at dim - 1; whole-pixel shortcut; tip-tilt planes evaluated from the two commands).  Four-parameter form:
 * A = (1 / G) [[cos t, sin t], [-sin t, cos t]], t = -A (dx, dy) ("Mirror mis-registration").
 * The object belongs to the context it was created with (reference: dmCompass.py:148-176). */
typedef struct aomarl_dmreg aomarl_dmreg;
/* Allocates the table for nenv environments of ctx's mirrors; it starts as the identity (dmCompass.py:148-176: the
 * reference's defaults dx = dy = theta = 0, G = 1).  Refuses a context with a pipelined frame or a prefetched reset in
 * flight.  Nothing is allocated afterwards. */
int aomarl_dmreg_create(aomarl_ctx *ctx, int nenv, aomarl_dmreg **out);
int aomarl_dmreg_destroy(aomarl_dmreg *r);
/* Rows of mirror `dm` for environments env_begin .. env_begin + env_count - 1 (dmCompass.py:148-176).  At: HOST
 * [env_count][6], copied before the call returns.  Refused by name: non-finite entries, |A_ij| > 4, |det A| outside
 * [1/4, 4], |t| beyond 4 dim of the mirror, a bad range or mirror index -- so that no accepted table takes a coordinate
 * near the int32 range; the kernel does not clamp.  The copy is ordered on `stream`, which is synchronised. */
int aomarl_dmreg_set(aomarl_dmreg *r, int env_begin, int env_count, int dm, const float *At, void *stream);
/* The same rows read back from the device into HOST At [env_count][6] (dmCompass.py:148-176 has no getter; the tests
 * do).  Synchronises `stream`. */
int aomarl_dmreg_get(aomarl_dmreg *r, int env_begin, int env_count, int dm, float *At, void *stream);
/* aomarl_raytrace_wfs (target = 0, writes st->wfs_phase) or aomarl_raytrace_target (target = 1, st->tar_phase) with
 * every mirror sampled through its row of the table (dmCompass.py:148-176); the atmosphere part and the
 * AOMARL_TRACE_* flags mean what they mean there.  One kernel launch: layers and mirrors in one pass, one store per
 * pixel.  Stack-array shapes a deferred apply_control left stale are materialised first.  Asynchronous on `stream`; no
 * synchronisation, read-back or allocation. */
int aomarl_dmreg_trace(aomarl_dmreg *r, aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count, int target,
                       int flags, void *stream);

/* Laser guide star on the Shack-Hartmann sensor ("Laser guide star"; the model is ao_marl_amd/lgs.py:
 * LgsModel and cone_trace_model).  The reference's host side is shesha/init/lgs_init.py; its native calls (lgs_init,
 * lgs_update, lgs_makespot, the convolution in comp_image, the cone in raytrace) are not in the reference tree.
 * Per (environment, sub-aperture k): the tile a = mask exp(i (2 pi / lambda phase - halfxy)), pdiam x pdiam, top-left
 * phase pixel (sub_x0[k], sub_y0[k]);  I = |fft2(a zero-padded to N)|^2;  J = I circularly convolved with the kernel
 * K_k [N][N];  sums of J over nrebin x nrebin blocks of the window of npix nrebin pixels centred on pixel N / 2 (the
 * unrolled binmap, geom_init.py:751);  times nphotons flux[k] / (sum of the window);  optional noise (the draw rule of the
 * Shack-Hartmann pixels, idx = flat index of the cube [nvalid][npix^2]);  centre of gravity
 * (sum v x / sum v - cog_offset) cog_scale, all x then all y, minus the reference slopes.
 * Arrays of the desc are HOST arrays, copied by create.  Sizes: pdiam = 16 with N = 64, and pdiam = 8 with N = 32; others
 * are refused by name. */
typedef struct {
  int32_t nenv, n, pdiam, N, npix, nrebin, nvalid;
  float lambda_um;   /* wavelength of the sensor in microns (the phase is in microns) */
  float nphotons;    /* photons per frame and full sub-aperture */
  float noise;       /* < 0: none; 0: photon noise; > 0: + read-out noise of that many electrons rms */
  float cog_offset, cog_scale;
  const float *mpupil;                     /* [n][n] */
  const float *halfxy;                     /* [pdiam][pdiam] */
  const float *flux;                       /* [nvalid] */
  const int32_t *sub_x0, *sub_y0;          /* [nvalid] */
} aomarl_lgs_desc;
typedef struct aomarl_lgs aomarl_lgs;
enum { AOMARL_LGS_NOISE = 1, AOMARL_LGS_WRITE_CUBE = 2 };
/* Allocates everything (sensors.d_wfs[i].d_gs.d_lgs.lgs_init, lgs_init.py:309: the native object of the reference);
 * nothing is allocated afterwards.  The kernels start as the impulse at (N / 2, N / 2) and the reference slopes as zero. */
int aomarl_lgs_create(const aomarl_lgs_desc *desc, aomarl_lgs **out);
int aomarl_lgs_destroy(aomarl_lgs *p);
/* K: HOST [nvalid][N][N], finite, not negative, each with a positive sum (lgs_init.py:198, p_wfs._lgskern, which the
 * reference uploads through lgs_init / lgs_update / lgs_makespot).  The device keeps, per sub-aperture, the table
 * Kt(sy, sx) = sum_j K(j) exp(+2 pi i j . s / N), |sy| <= pdiam - 1, 0 <= sx <= pdiam - 1, formed here in double.
 * Synchronises the device. */
int aomarl_lgs_set_kernels(aomarl_lgs *p, const float *K);
/* ref: HOST [2 nvalid], subtracted from every slope vector; NULL: zero (the reference's centroider's set_ref).
 * Synchronises the device. */
int aomarl_lgs_set_ref(aomarl_lgs *p, const float *ref);
/* aomarl_raytrace_wfs through the cone (wfs_init.py:170-185, the gsalt terms of the offsets, and the native raytrace's
 * cone): pixel (x, y) of the sensor's grid samples layer l at ((x, y) + (wxo, wyo)) + dm1[l] ((x, y) - (n - 1) / 2),
 * dm1[l] = delta_l - 1 = -alt_l / gsalt (HOST [nlayers], in (-1, 0]), one fused multiply-add per coordinate, bilinear by
 * the trace's rule; mirrors are traced as aomarl_raytrace_wfs traces them.  Writes st->wfs_phase of environments
 * env_begin .. env_begin + env_count - 1; flags: AOMARL_TRACE_ATMOS | _DMS | _RESET.  dm1 = 0 gives aomarl_raytrace_wfs
 * to the bit.  Asynchronous on `stream`; no synchronisation, read-back or allocation. */
int aomarl_lgs_trace(aomarl_lgs *p, aomarl_ctx *ctx, aomarl_state *st, const float *dm1, int nlayers, int env_begin,
                     int env_count, int flags, void *stream);
/* The image and slopes (the reference's comp_image with its LGS convolution, then the centroider).  phase: DEVICE
 * [nenv][n * n] microns; image: DEVICE [nenv][nvalid][npix^2], written with AOMARL_LGS_WRITE_CUBE; slopes: DEVICE
 * [nenv][2 nvalid]; rows of the environments measured are written.  flags & AOMARL_LGS_NOISE: the desc's noise is drawn
 * with seeds[e] and frame[e] (DEVICE [nenv], as aomarl_state has them) and frame[e] advances by one.  One workgroup per
 * (environment, sub-aperture), no atomics, every sum in a fixed order: the bits do not depend on how the environments
 * are split into calls.  Asynchronous on `stream`; no allocation, no read-back. */
int aomarl_lgs_measure(aomarl_lgs *p, const float *phase, int env_begin, int env_count, int flags, const uint32_t *seeds,
                       uint32_t *frame, float *image, float *slopes, void *stream);

/* Laser tomography: a constellation of up to AOMARL_TOMO_MAX_STARS guide stars on the Shack-Hartmann sensor (DESIGN.md,
 * "Laser tomography"; the model is ao_marl_amd/tomography.py: tomo_trace_model and slope_covariance).  The reference has
 * the host wiring alone (shesha/ao/tomo.py); its covariances live in an external library that is not in its tree. */
#define AOMARL_TOMO_MAX_STARS 8
typedef struct {
  int32_t nstars, nlayers;
  const float *off;   /* HOST [nstars][nlayers][2]: the layer offset (x, y) of star k, wfs offset + theta_k alt_l / pupixsize */
  const float *dm1;   /* HOST [nstars][nlayers]: delta_kl - 1 = -alt_l / gsalt_k, in (-1, 0] */
} aomarl_tomo_desc;
/* aomarl_lgs_trace for every star of an environment in one launch: pixel (x, y) of the sensor's grid samples layer l for
 * star k at ((x, y) + off_kl) + dm1_kl ((x, y) - (n - 1) / 2), one fused multiply-add per coordinate, bilinear by the
 * trace's rule; the mirrors (all in the pupil: the same value for every star) are evaluated once per pixel and added to
 * each star's sum in controller order.  planes: DEVICE [nenv][nstars][n * n]; plane (e, k) has the bits aomarl_lgs_trace
 * gives with star k's numbers.  flags: AOMARL_TRACE_ATMOS | _DMS | _RESET | _MASK.  Refused by name: nstars outside 1..8,
 * a layer count that differs from the context's, non-finite offsets, dm1 outside (-1, 0], a footprint (the coordinate at
 * the grid's corners) outside [0, dim - 1] of a screen, a null pointer, a bad range, a pipelined frame or a prefetched
 * reset in flight.  Asynchronous on `stream`; no synchronisation, read-back or allocation. */
int aomarl_tomo_trace(aomarl_ctx *ctx, aomarl_state *st, const aomarl_tomo_desc *desc, float *planes, int env_begin,
                      int env_count, int flags, void *stream);
/* The covariance in arcsec^2 of two-point slopes between directions (tomography.slope_covariance), in double:
 *   out[(2 a + e) n_row + i][(2 b + f) n_col + j] = sum_l w_l sum_{s, s' = +-1} (-s s' / 2)
 *       rodconan(|u_i^{a,l} - u_j^{b,l} + s delta_al d / 2 e - s' delta_bl d / 2 f|, L0_l),
 *   u_i^{a,l} = delta_al p_i + alt_l theta_a,  delta_al = 1 - alt_l / gsalt_a,  theta in radians (arcsec 2 pi / 1296000),
 *   w_l = (1e-6 206265 / d)^2 r0_l^(-5/3) (0.5 / 2 pi)^2;  layers outer, then the taps (+,+), (+,-), (-,+), (-,-).
 * Every array of the desc is a HOST array, copied by the call: points in metres, stars [k][3] = (x arcsec, y arcsec,
 * gsalt m; infinity: a natural star), layers [nlayers][3] = (alt m, r0_l m, L0_l m).  out: DEVICE double
 * [2 n_row k_row][2 n_col k_col].  One thread per element, no atomics: the bits do not depend on the launch.  Allocates
 * and frees its tables and synchronises `stream` (a calibration call). */
typedef struct {
  int32_t n_row, n_col, k_row, k_col, nlayers;
  double d;                                   /* side of a sub-aperture in metres */
  const double *row_px, *row_py, *col_px, *col_py;
  const double *row_stars, *col_stars, *layers;
} aomarl_tomo_cov_desc;
int aomarl_tomo_cov(const aomarl_tomo_cov_desc *desc, double *out, void *stream);

/* Science field: Strehl and long-exposure PSF window in any number of directions per environment ("Science
 * field"; the model is ao_marl_amd/field.py: field_offsets, field_trace_model, FieldModel).  Natural stars: no cone.
 * The mirrors all sit in the pupil and are traced by the target's rule: their value at a pixel is the same for every
 * direction.  The PSF grid (npsf, strehl_halfwin, ref_peak) is the context's; one wavelength per object. */
#define AOMARL_FIELD_MAX_DIRS 16 /* directions per launch; a field with more runs as consecutive launches */
typedef struct {
  int32_t ndir, nlayers;
  const float *off;  /* HOST [ndir][nlayers][2]: the layer offset (x, y) of direction d on the pupil (pupdiam) grid,
                        the target's offset + theta_d alt_l / pupixsize; copied by aomarl_field_create */
  float inv_lambda;  /* 1 / wavelength in microns */
} aomarl_field_desc;
typedef struct aomarl_field aomarl_field;
/* The object owns record [nenv][ndir][8] (the slots of aomarl_state.strehl, per direction), le [nenv][ndir][W][W]
 * (W = 2 strehl_halfwin, the long-exposure sum) and its workspaces; everything is allocated here, zeroed.  Refused by
 * name: ndir < 1, a layer count that differs from the context's, non-finite offsets, a footprint (the coordinate at the
 * pupil grid's corners) outside [0, dim - 1] of a screen, a mirror that is not in the pupil (at altitude), null
 * pointers, nenv < 1, nenv ndir pupdiam^2 beyond 2^31 - 1, inv_lambda non-finite or <= 0. */
int aomarl_field_create(aomarl_ctx *ctx, int nenv, const aomarl_field_desc *desc, aomarl_field **out);
int aomarl_field_destroy(aomarl_field *f);
/* For every environment of the range and every direction: the phase of the state as it stands, traced bilinearly by the
 * trace's rule through the layers (flags & AOMARL_TRACE_ATMOS) and the mirrors (AOMARL_TRACE_DMS), straight into the
 * windowed PSF |DFT_npsf(spupil exp(2 pi i phase inv_lambda))|^2 on [-hw, hw)^2, the phase variance over the lit pixels
 * and the sinc fit; committed into the object's record and long-exposure sum (what aomarl_comp_strehl does to
 * st->strehl / st->le_img).  No phase plane is written; st->tar_phase, st->strehl, st->le_img and the pending PSF slot
 * are not touched; deferred stack-array shapes are materialised first (aomarl_target_image).  No atomics, every sum in
 * a fixed order: the record and the window of direction d of environment e have the same bits however the environments
 * are split into calls, however many other directions the field has and whichever launch d falls into.  Refused by
 * name: null pointers, a state of another size, a bad range, unknown flags, a pipelined frame or a prefetched reset in
 * flight.  Asynchronous on `stream`; no synchronisation, read-back or allocation. */
int aomarl_field_observe(aomarl_field *f, aomarl_ctx *ctx, aomarl_state *st, int env_begin, int env_count, int flags,
                         void *stream);
/* The traced planes alone: planes DEVICE [nenv][ndir][pupdiam^2], flags AOMARL_TRACE_ATMOS | _DMS | _RESET | _MASK as
 * for aomarl_tomo_trace (_MASK multiplies by spupil).  Direction offsets that are whole pixels give
 * aomarl_raytrace_target's bits. */
int aomarl_field_trace(aomarl_field *f, aomarl_ctx *ctx, aomarl_state *st, float *planes, int env_begin, int env_count,
                       int flags, void *stream);
/* Zero the record and the long-exposure sum of the environments of the range. */
int aomarl_field_reset(aomarl_field *f, int env_begin, int env_count, void *stream);
/* Device pointers to record and le (either may be NULL); do_fit: first solve the long exposure's sinc fit into slot 7
 * of every record (on demand, like aomarl_strehl_fit), asynchronously on `stream`. */
int aomarl_field_get(aomarl_field *f, int do_fit, float **record, float **le, void *stream);

/* Multi-conjugate AO: up to AOMARL_MCAO_MAX_MIRRORS stack-array mirrors conjugated to altitudes h_m >= 0, owned by the
 * object and not by the context ("Multi-conjugate AO"; the model is ao_marl_amd/mcao.py: altitude_mirror,
 * mirror_shape_model, mirror_offsets, mirrors_add_model, delay_line_model).  Every guide star and every science direction
 * sees a mirror at altitude through its own footprint. */
#define AOMARL_MCAO_MAX_MIRRORS 2
#define AOMARL_MCAO_MAX_DIRS 8 /* directions (stars) per aomarl_mcao_add */
typedef struct {
  float alt;                    /* metres, >= 0 */
  int32_t dim;                  /* the side of the mirror's plane in pupil pixels */
  int32_t pitch, i1min, j1min;  /* the lattice: the patch of cell (gx, gy) starts at (i1min + pitch gx, j1min + pitch gy) */
  int32_t gw, gh;               /* lattice cells */
  int32_t ss, nact;             /* the profile's length; actuators */
  const int32_t *grid;          /* HOST [gh][gw]: the cell's actuator, or -1 */
  const float *prof;            /* HOST [ss]: the separable profile, influence(a, b) = prof[a] prof[b] microns per unit */
} aomarl_mcao_mirror;
typedef struct {
  int32_t nmirrors;
  aomarl_mcao_mirror mirrors[AOMARL_MCAO_MAX_MIRRORS];
} aomarl_mcao_desc;
/* How `ndir` directions look at the mirrors: pixel (x, y) of a grid of side nn samples mirror m for direction k at
 * ((x, y) + off_km) + dm1_km ((x, y) - (nn - 1) / 2), one fused multiply-add per coordinate (aomarl_tomo_trace's layer
 * rule), bilinear by the trace's rule for a plain plane: zero outside, the last line clamped. */
typedef struct {
  int32_t ndir;
  const float *off; /* HOST [ndir][nmirrors][2] */
  const float *dm1; /* HOST [ndir][nmirrors]: -h_m / gsalt_k in (-1, 0]; 0: a natural star, a science direction */
} aomarl_mcao_view;
typedef struct aomarl_mcao aomarl_mcao;
/* The object owns com, com1, com2, voltage [nenv][nact_total] (the mirrors' actuators one after the other) and the planes
 * [nenv][nmirrors][dim_max^2] (mirror m uses the first dim_m^2 floats of its slot, row length dim_m); all allocated here,
 * zeroed.  Refused by name: nmirrors outside 1..2, alt negative or not finite, a lattice that leaves the plane, grid
 * entries outside -1..nact - 1, a profile longer than the shape kernel's patch of lattice cells, null pointers, nenv < 1,
 * planes beyond 2^31 - 1 elements. */
int aomarl_mcao_create(aomarl_ctx *ctx, int nenv, const aomarl_mcao_desc *desc, aomarl_mcao **out);
int aomarl_mcao_destroy(aomarl_mcao *m);
/* Device pointers to the commands, the delayed voltages and the planes (each may be NULL). */
int aomarl_mcao_com(aomarl_mcao *m, float **com, float **voltage, float **planes);
/* volts == NULL: the delay line, voltage = wa com + wb com1 + wc com2 with the context's delay weights, com2 <- com1,
 * com1 <- com (aomarl_apply_control's expression and order), then every mirror's plane from the voltages.  volts: DEVICE
 * [env_count][nact_total], shaped directly (the calibration's pokes, like aomarl_comp_dm_shape); the delay line is not
 * touched.  No atomics, every sum in a fixed order.  Asynchronous on `stream`. */
int aomarl_mcao_apply(aomarl_mcao *m, aomarl_ctx *ctx, int env_begin, int env_count, const float *volts, void *stream);
/* Zero the commands, the delay line, the voltages and the planes of the environments of the range. */
int aomarl_mcao_reset(aomarl_mcao *m, int env_begin, int env_count, void *stream);
/* planes[e][k] += sum_m sample(mirror m) for the ndir directions of the view, in mirror order, behind whatever the plane
 * holds; planes: DEVICE [nenv][ndir][nn^2] with nn the context's n (the sensor's grid; what aomarl_tomo_trace left) or
 * pupdiam (with ndir = 1: the state's tar_phase).  flags: AOMARL_TRACE_MASK multiplies the result by mpupil (nn = n) or
 * spupil (nn = pupdiam).  Plane (e, k) has the same bits however many other directions the call has and however the
 * environments are split into calls.  Refused by name: ndir outside 1..8 or different from the view's, nn neither n nor
 * pupdiam, non-finite offsets, dm1 outside (-1, 0], a footprint (the coordinate at the grid's corners) outside
 * [0, dim_m - 1], null pointers, a bad range, unknown flags, planes beyond 2^31 - 1 elements, a pipelined frame or a
 * prefetched reset in flight.  Asynchronous on `stream`; no synchronisation, read-back or allocation. */
int aomarl_mcao_add(aomarl_mcao *m, aomarl_ctx *ctx, const aomarl_mcao_view *view, float *planes, int ndir, int nn,
                    int env_begin, int env_count, int flags, void *stream);
/* The science field through the mirrors: from now on aomarl_field_observe and aomarl_field_trace add, under
 * AOMARL_TRACE_DMS and behind the pupil mirrors, the planes of `m` as they stand, per direction, by aomarl_mcao_add's
 * sampling with dm1 = 0 on the pupil grid.  view: one entry per direction of the field (copied).  The object `m` must
 * outlive the attachment.  A field without attached mirrors runs what it ran before.  Refused by name: null pointers,
 * environment counts that differ, a view whose direction count differs from the field's, dm1 != 0, non-finite offsets, a
 * footprint outside [0, dim_m - 1]. */
int aomarl_field_attach_mirrors(aomarl_field *f, aomarl_mcao *m, const aomarl_mcao_view *view);
int aomarl_field_detach_mirrors(aomarl_field *f);

#ifdef __cplusplus
}
#endif
#endif
