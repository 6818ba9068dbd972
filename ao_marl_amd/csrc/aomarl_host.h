// aomarl_host.h -- host-side pieces shared by the translation units of libaomarl_hip.so (aomarl_capi.hip: context,
// atmosphere / control kernels and their entry points; aomarl_frame.hip, aomarl_wfs.hip, aomarl_target.hip: the frame
// kernel and the staged sensor and target kernels, launched through aomarl_frame_host.h / aomarl_stage_host.h; aomarl_capi_dmreg.hip, aomarl_lgs.hip, aomarl_tomo.hip,
// aomarl_field.hip, aomarl_mcao.hip: what traces on a context, through aomarl_env_host.h; aomarl_denoise.hip: the denoiser;
// aomarl_denoise_train.hip: its training step; aomarl_sac.hip: the learner's update and the grouped GEMM; aomarl_roket.hip: the ROKET filter bank; aomarl_psfrec.hip: the PSF reconstruction; aomarl_groot.hip: the GROOT covariance model; aomarl_modopti.hip: the modal-gain filter bank; aomarl_predictor.hip: the modal predictor).  Not part of the C ABI: hidden visibility.
#pragma once
#include "aomarl_dev.h"

#define AOMARL_LOCAL __attribute__((visibility("hidden")))

// sets this thread's last-error text (aomarl_last_error), returns 1
AOMARL_LOCAL int fail(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

#define HIPCHK(x)                                                                            \
  do {                                                                                       \
    hipError_t _e = (x);                                                                     \
    if (_e != hipSuccess) return fail("%s failed: %s (%s:%d)", #x, hipGetErrorString(_e),    \
                                      __FILE__, __LINE__);                                   \
  } while (0)
#define LAUNCHCHK()                                                                          \
  do {                                                                                       \
    hipError_t _e = hipGetLastError();                                                       \
    if (_e != hipSuccess) return fail("kernel launch failed: %s (%s:%d)",                    \
                                      hipGetErrorString(_e), __FILE__, __LINE__);            \
  } while (0)

// launches per arithmetic family since aomarl_arith_reset (bench.py builds its `dtype` from them)
enum { AR_FRAME_F32 = 0, AR_FRAME_SPLIT, AR_GEMM_F32, AR_GEMM_SPLIT, AR_DENOISE_F32, AR_DENOISE_SPLIT, AR_ACTOR_F32, AR_N };
extern AOMARL_LOCAL unsigned long long g_arith[AR_N];
extern AOMARL_LOCAL int g_precision;           // process-wide default of every family (aomarl_set_precision)

// round 1's general batched product (aomarl_capi_composites.hip): rows that are not 16-byte aligned, accumulation into C
AOMARL_LOCAL int gemm_batched_launch(int batch, int transA, int transB, int M, int N, int K, const float *A, int lda,
                                     long long strideA, const float *B, int ldb, long long strideB,
                                     const float *bias, long long strideBias, float *C, int ldc, long long strideC,
                                     int relu, int accumulate, const float *mask, int ldm, long long strideM,
                                     hipStream_t s);
// one launch of the grouped kernel (aomarl_gemm_g.h, instantiated in aomarl_sac.hip alone): C[g] = act(opA(A[g]) opB(B[g]) +
// bias[g]), zero where mask[m][n] <= 0 (rows ldm apart, one mask for every group; null: none); ak / bk: the operand is
// contiguous along k
AOMARL_LOCAL int gemm_g_batched(int batch, bool ak, bool bk, int M, int N, int K, const float *A, int lda, long long sA,
                                const float *B, int ldb, long long sB, const float *bias, long long sBias, float *C, int ldc,
                                long long sC, int relu, const float *mask, int ldm, hipStream_t s);
// gemm_p_launch out of line: one launch of k_gemm_p (aomarl_gemm_p.h, instantiated in the environment's unit alone) with
// a configuration of gemm_p_pick (aomarl_gemm_p_host.h); false: not launched
struct GemmPCfg;
AOMARL_LOCAL bool gemm_p_launch_cfg(const GemmPCfg &c, int M, int N, int K, float alpha, const float *A, int lda,
                                    const float *B, int ldb, float beta, float *C, int ldc, float *P, int xcd, hipStream_t s);

// the on-line modal-gain optimiser (aomarl_modopti.hip) as aomarl_do_control sees it while one is attached
// (aomarl_modopti_online_attach, aomarl_capi_stages.hip): p = v2m . voltage goes into mo_online_p, mo_online_pol writes
// x = e + p into the ring row of this frame, mo_online_advance counts the frame and runs the bank / the apply the
// schedule asks for (mgain_dev: the context's modal gains, written by the apply as float(G / gain))
struct aomarl_modopti_online;
AOMARL_LOCAL void mo_online_dims(const aomarl_modopti_online *m, int *nenv, int *nmodes, int *rows);
AOMARL_LOCAL const void *mo_online_owner(const aomarl_modopti_online *m);
AOMARL_LOCAL void mo_online_set_owner(aomarl_modopti_online *m, const void *owner);
AOMARL_LOCAL float *mo_online_p(aomarl_modopti_online *m);
AOMARL_LOCAL int mo_online_pol(aomarl_modopti_online *m, const float *e, int lde, hipStream_t s);
AOMARL_LOCAL int mo_online_advance(aomarl_modopti_online *m, float *mgain_dev, float gain, hipStream_t s, bool *applied);
// k_mo_pol for any consumer of the pseudo-open-loop modes: x[nenv][nm] = e (rows lde apart) + p[nenv][nm]
AOMARL_LOCAL int mo_pol(const float *e, int lde, const float *p, int nenv, int nm, float *x, hipStream_t s);

// the modal predictor (aomarl_predictor.hip) as aomarl_do_control and aomarl_rl_control_modes see it while one is
// attached (aomarl_predictor_attach): p = v2m . voltage goes into pred_p, x = e + p into pred_x, pred_frame runs the
// filter on that row and writes c into pred_c ([nenv][nmodes]) and into `modes` (rows ldm apart, the GEMM operand)
struct aomarl_predictor;
AOMARL_LOCAL void pred_dims(const aomarl_predictor *p, int *nenv, int *nmodes);
AOMARL_LOCAL const void *pred_owner(const aomarl_predictor *p);
AOMARL_LOCAL void pred_set_owner(aomarl_predictor *p, const void *owner);
AOMARL_LOCAL float *pred_p(aomarl_predictor *p);
AOMARL_LOCAL float *pred_x(aomarl_predictor *p);
AOMARL_LOCAL const float *pred_c(const aomarl_predictor *p);
AOMARL_LOCAL int pred_frame(aomarl_predictor *p, float *modes, int ldm, hipStream_t s);
