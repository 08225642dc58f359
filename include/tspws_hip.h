/*
 * tspws_hip.h -- the thin C-ABI HIP layer under tspws_main().
 *
 * Plain C types only (pointers, sizes, scalars); every `d_` pointer is a HIP
 * device pointer on the plan's device, `stream` is a hipStream_t passed as
 * void* (NULL = the default stream).  All functions return 0 on success or a
 * TSPWS_E_* code; tspws_hip_last_error() gives the text.  Nothing here exists
 * in the reference (it has no device code): each entry point names the
 * reference routine whose work it takes over, paths relative to
 * /root/reference/src.
 *
 * Coefficient containers are the reference's ragged [S][N_s] layout
 * (FWTa/wavelet_mem_v7.c:78-106) flattened: scale s starts at coef_off[s],
 * N_s = ceil(N / D_s); complex values are interleaved (re, im) doubles.
 */
#ifndef TSPWS_HIP_H
#define TSPWS_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "ts_pws1f_lib.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
	TSPWS_OK        = 0,
	TSPWS_E_ARG     = -1, /* NULL / inconsistent argument (tspws_main returns -1 for NULL too)   */
	TSPWS_E_NOMEM   = 4,  /* host or device allocation failed (reference code, ts_pws1f_lib.c:199) */
	TSPWS_E_NODEV   = 5,  /* no usable HIP device or kernel image                               */
	TSPWS_E_HIP     = 6,  /* a HIP runtime call failed                                          */
	TSPWS_E_FRAME   = 7   /* frame cannot be built (bad family id, wavelet longer than trace)   */
};

typedef struct tspws_hip_plan tspws_hip_plan;

typedef struct {
	int      type;          /* -1 / -2 / -3                                     */
	unsigned S, V, J, N;    /* scales, voices, octaves, trace length            */
	double   s0, b0, w0;    /* as passed to plan_create                         */
	double   Cpsi;          /* admissibility constant                           */
	size_t   ncoef;         /* sum of N_s  (complex coefficients per trace)     */
	size_t   ntaps;         /* sum of L_s  (complex taps; the dual has as many) */
	int      device;
} tspws_hip_frame_info;

/* ---- runtime helpers so that the C host needs no HIP headers ------------------ */
int         tspws_hip_device_count(void);
const char *tspws_hip_last_error(void);
int  tspws_hip_alloc(void **d_ptr, size_t bytes, int device);
int  tspws_hip_free(void *d_ptr);
int  tspws_hip_upload(void *d_dst, const void *h_src, size_t bytes, void *stream);
int  tspws_hip_download(void *h_dst, const void *d_src, size_t bytes, void *stream);
int  tspws_hip_zero(void *d_ptr, size_t bytes, void *stream);
int  tspws_hip_sync(void *stream);

/* ---- parameters and plan ------------------------------------------------------ */

/* Resolve w0 / V / b0 / s0 / J from the user's knobs, rewriting *p in place.
 * Takes over ts_pws1f_lib.c:91-124 (host arithmetic, bit-for-bit the same rules). */
void tspws_resolve_params(t_tsPWS *p, unsigned nsamp, float dt);

/* Build the frame on `device`: geometry tables on the host, taps / dual taps generated
 * by a device kernel, container offsets.  Takes over CreateWaveletFamily
 * (FWTa/wavelet_def_v7.c:204-295) and the container set-up (wavelet_mem_v7.c:78-106).
 * Argument meaning and order follow CreateWaveletFamily(type, J, V, N, s0, b0, -, w0, uni). */
int  tspws_hip_plan_create(tspws_hip_plan **plan, int type, unsigned J, unsigned V, unsigned N,
                           double s0, double b0, double w0, int uni, int device);
void tspws_hip_plan_destroy(tspws_hip_plan *plan);   /* DestroyWaveletFamily, wavelet_def_v7.c:341 */
int  tspws_hip_plan_info(const tspws_hip_plan *plan, tspws_hip_frame_info *info);
/* host copies of the per-scale tables; any pointer may be NULL */
int  tspws_hip_plan_tables(const tspws_hip_plan *plan, double *scale, unsigned *L, int *c, int *cd,
                           unsigned *D, unsigned *Ns);
/* device -> host copy of the (re,im) tap tables, 2*ntaps doubles each (tests) */
int  tspws_hip_plan_taps(const tspws_hip_plan *plan, double *h_w, double *h_wd);

/* ---- trace prologue (in place, float) ----------------------------------------- */
/* fold: x[n] = x[max-1-n] = 0.5f*(x[n]+x[max-1-n]).   ts_pws1f_lib.c:76-86 */
int  tspws_hip_fold(float *d_sigall, size_t mtr, size_t max, size_t ld, void *stream);
/* remove each trace's mean (FP64 sum, float subtraction).   ts_pws1f_lib.c:159-169 */
int  tspws_hip_remove_mean(float *d_sigall, size_t mtr, size_t max, size_t ld, void *stream);

/* ---- stage 1 of the two-stage stack -------------------------------------------- */
/* P[g][n] (+)= sum of this shard's traces whose GLOBAL index i = first + local falls in group
 * g = floor(i*Kmax/mtr_global); P is [Kmax][ldP] doubles and is overwritten (rows of groups the
 * shard does not touch become 0).  Takes over partial_linear_stacks, ts_pws1f_lib.c:866-881.
 * This is the HBM-streaming kernel: every input sample is read exactly once. */
int  tspws_hip_partial_stacks(tspws_hip_plan *plan, const float *d_sigall, size_t ld,
                              size_t mtr_local, size_t first, size_t mtr_global, unsigned Kmax,
                              double *d_P, size_t ldP, void *stream);

/* Same, restricted to the groups [g_begin, g_end): only those rows of P are written.  Lets a multi-GPU caller start the
 * all-reduce of the first groups while the later ones are still being streamed. */
int  tspws_hip_partial_stacks_range(tspws_hip_plan *plan, const float *d_sigall, size_t ld,
                                    size_t mtr_local, size_t first, size_t mtr_global, unsigned Kmax,
                                    unsigned g_begin, unsigned g_end, double *d_P, size_t ldP, void *stream);

/* ---- frame transforms ------------------------------------------------------------ */
/* Forward frame CWT of ntr real traces (row stride ld elements) into d_Y[ntr][ncoef] complex.
 * Takes over complex_1D_wavelet_dec (wavelet_v7.c:43-64) -> cdotx_dc (cdotx.c:35-72). */
int  tspws_hip_forward_f64(tspws_hip_plan *plan, const double *d_x, size_t ntr, size_t ld, double *d_Y, void *stream);
int  tspws_hip_forward_f32(tspws_hip_plan *plan, const float  *d_x, size_t ntr, size_t ld, double *d_Y, void *stream);
/* The same coefficients through the SPECTRAL engine (csrc/spectral.hip): only the scales of the frame's spectral set for octaves of at
 * most nsmax outputs -- [tspws_hip_spectral_first_scale(plan, nsmax), tspws_hip_spectral_end_scale(plan)) -- are written, the rest of
 * d_Y[ntr][ncoef] is left alone.  Exact for those scales because the reference's FIR is a circular correlation (cdotx.c:35-72): for N a
 * power of two it is the transform's own (D divides N); for any other N >= 1024 it is evaluated as a linear correlation over a window of
 * the trace's periodic extension, tspws_hip_spectral_transform_length(plan) >= N + L - 1 samples long -- scales whose filters do not fit
 * that window lie at and behind tspws_hip_spectral_end_scale (S for most frames).  Returns TSPWS_E_ARG when the frame has no such set
 * (N < 1024, decimations that are not powers of two >= 8, ...). */
unsigned tspws_hip_spectral_first_scale(const tspws_hip_plan *plan, unsigned nsmax);
unsigned tspws_hip_spectral_end_scale(const tspws_hip_plan *plan);
unsigned tspws_hip_spectral_transform_length(const tspws_hip_plan *plan);
/* First scale of the spectral set a single-stage batch of ntr traces gets by the library's own rule (S: FIR kernels only): batches of
 * >= 64 traces and >= 1 M samples (or >= 256 traces) send the octaves with D >= 32 (two-voice frames: D >= 16) through the spectrum;
 * TSPWS_ENGINE=fir / spectral pins the choice. */
unsigned tspws_hip_spectral_choice(const tspws_hip_plan *plan, size_t ntr);
int  tspws_hip_forward_spectral_f64(tspws_hip_plan *plan, const double *d_x, size_t ntr, size_t ld, double *d_Y, unsigned nsmax, void *stream);
int  tspws_hip_forward_spectral_f32(tspws_hip_plan *plan, const float  *d_x, size_t ntr, size_t ld, double *d_Y, unsigned nsmax, void *stream);
/* Real part of the inverse frame transform of nrec coefficient sets d_Y[nrec][ncoef] into
 * d_x[nrec][N] doubles.  Takes over Re_complex_1D_wavelet_rec (wavelet_v7.c:124-150) ->
 * re_cdotx_upsampling_cc (cdotx.c:305-340) / re_cdotx_cc (cdotx.c:176-211). */
int  tspws_hip_inverse(tspws_hip_plan *plan, const double *d_Y, size_t nrec, double *d_x, void *stream);
/* How tspws_hip_inverse launches this plan's frame (read-only, no device work): the work list of the polyphase kernel k_inv_poly and the
 * wave ranges of its instantiations, so that a test can assert the route it means to take.  Waves [0, waves_lds) take the LDS-staged
 * instantiation when a call has two or more pairs of sets (the per-lane one otherwise), [waves_lds, waves_fast) the per-lane / wave-uniform
 * one, [waves_fast, waves) the three-frame GEN one (decimations that do not divide N). */
typedef struct {
	unsigned items;      /* work items of the launch list                                                        */
	unsigned per_scale;  /* 1: one item per scale (the short-frame form), 0: one per decimation octave           */
	unsigned waves;      /* waves of the whole list                                                              */
	unsigned waves_lds;  /* ... of which the first waves_lds are LDS-staged in calls with two or more pairs       */
	unsigned waves_fast; /* waves of the items whose D divides N (the GEN waves are waves - waves_fast)            */
	unsigned generic;    /* 1: k_inverse_generic is in force instead (TSPWS_INV_GENERIC=1 of the sweeps build)     */
} tspws_hip_inverse_info_t;
int  tspws_hip_inverse_info(const tspws_hip_plan *plan, tspws_hip_inverse_info_t *info);

/* ---- band rows: the reconstruction per range of scales, with its quadrature ------------ */
/* The reconstruction is a sum over the S scales (x^ = sum_s x_s, x_s = gain_s D_s sum Re(conj(wd_s[l]) Y_s[..]): csrc/inv_poly.h).  A band
 * is a half-open scale range [s_begin, s_end), 0 <= s_begin <= s_end <= S; bands of one table may overlap, cut a decimation octave between
 * two voices, or be empty.  For a coefficient set Y and a band r, in FP64,
 *   X_r = sum_{s in band} x_s,   Q_r = sum_{s in band} q_s   (added in increasing s),   E_r[n] = hypot(X_r[n], Q_r[n])
 * where q_s is x_s with Im in place of Re: the real row of the set -i Y = (Im Y, -Re Y), i.e. the band-limited signal's quadrature, and E_r
 * its envelope.  The row of a band does not depend on which other bands the table holds, bit for bit: every scale inside at least one
 * band is one work item of the polyphase kernel, whatever the table, and a combining kernel adds a band's scale rows in increasing s. */
typedef struct { unsigned s_begin, s_end; } tspws_band;
#define TSPWS_MAX_BANDS 1024u
/* X_r (d_re) and Q_r (d_im; NULL: real rows only, no quadrature work) of nset coefficient sets d_Y[nset][ncoef], as [nset][R][N] doubles.
 * Each set is read once.  An empty band gives zero rows; R = 0 or nset = 0 returns 0 and does nothing.  A NULL plan / d_Y / h_bands / d_re,
 * s_end > S, s_begin > s_end and R > TSPWS_MAX_BANDS return TSPWS_E_ARG ("inverse_bands: ...") before any device work, outputs untouched;
 * the checks that need no plan come first.
 * The scale rows of a batch of sets (scales inside a band x N doubles per set, twice that with the quadrature) stay within TSPWS_PART_MB.
 * The work is ordered on `stream`; a call whose band table differs from the plan's previous one first waits for `stream` (the device copy
 * of the table is the plan's).  Sweeps builds: TSPWS_INV_GENERIC does not apply (band rows always take the polyphase kernel). */
int  tspws_hip_inverse_bands(tspws_hip_plan *plan, const double *d_Y, size_t nset, const tspws_band *h_bands, unsigned R,
                             double *d_re, double *d_im, void *stream);
/* Host rule, no device: bands of centre frequencies.  fc_s = w0 / (2 PI dt scale_s) (the reference's relation between fmin and the largest
 * scale, ts_pws1f_lib.c:112, operations in that order; decreasing in s, written to fc[S] unless NULL); band r = the scales with
 * f_lo[r] <= fc_s < f_hi[r] -- a contiguous range, and bands with shared edges partition the scales between the outer edges.  A band above
 * or below every fc_s is empty.  A NULL scale / f_lo / f_hi / bands (with R > 0), a non-finite edge, f_lo > f_hi and dt <= 0 (or not
 * finite) return TSPWS_E_ARG. */
int  tspws_bands_from_frequencies(const double *scale, unsigned S, double w0, double dt, const double *f_lo, const double *f_hi, unsigned R,
                                  tspws_band *bands, double *fc);

/* ---- stacks in the time-scale domain ----------------------------------------------- */
/* ST += sum_b Y_b ; PS += sum_b Y_b/|Y_b| (non-unit quotients skipped); zero_first clears
 * ST/PS before.  The loop body of ts_pws1f_lib.c:486-494 / :897-904. */
int  tspws_hip_accumulate(tspws_hip_plan *plan, const double *d_Y, size_t ntr, double *d_ST, double *d_PS,
                          int zero_first, void *stream);
/* forward + accumulate of K double-precision partial stacks.  tspws_stacks_double, :885-906 */
int  tspws_hip_stacks_double(tspws_hip_plan *plan, const double *d_P, unsigned K, size_t ldP,
                             double *d_ST, double *d_PS, void *stream);
/* forward + accumulate of mtr float traces (ST/PS are cleared first).  tspws_stacks_float, :466-499 */
int  tspws_hip_stacks_float(tspws_hip_plan *plan, const float *d_sigall, size_t mtr, size_t ld,
                            double *d_ST, double *d_PS, void *stream);
/* OUT = ST * weight(PS).  wu==2 && unbiased -> tspws_unbiased (:965-984) else tspws_biased (:909-943) */
int  tspws_hip_weight(tspws_hip_plan *plan, double *d_OUT, const double *d_ST, const double *d_PS,
                      unsigned K, unsigned M, double wu, int unbiased, void *stream);
/* ls[n] = (float)x_st[n] / mtr (float division), tsPWS[n] = (float)x_out[n].   :233-241 */
int  tspws_hip_epilogue(float *d_ls, float *d_tsPWS, const double *d_x_st, const double *d_x_out,
                        size_t N, unsigned mtr, void *stream);

/* ---- whole call on HBM-resident traces ------------------------------------------------ */
/* What tspws_main does between reading `in` and writing `out`, for one shard of traces that
 * already sits in device memory.  `p` must be resolved (tspws_resolve_params) and the plan
 * built from it.  Split in two so that a multi-GPU caller can sum the shard results between
 * the halves (one all-reduce of tspws_hip_reduce_buffer):
 *   _local : two-stage  -> partial stacks of the shard        (reduce buffer = P[Kmax][N])
 *            single     -> ST and PS of the shard's traces    (reduce buffer = ST||PS)
 *   _finish: (two-stage: forward+accumulate of the K partials,) weight, two inverses, epilogue.
 * d_ls / d_tsPWS receive `max` floats each. */
int  tspws_hip_stack_local(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld,
                           size_t mtr_local, size_t first, size_t mtr_global, void *stream);
int  tspws_hip_reduce_buffer(tspws_hip_plan *plan, const t_tsPWS *p, size_t mtr_global,
                             double **d_buf, size_t *ndoubles);
int  tspws_hip_stack_finish(tspws_hip_plan *plan, const t_tsPWS *p, size_t mtr_global,
                            float *d_ls, float *d_tsPWS, void *stream);

/* The finish stage in pieces, for callers that overlap it with the reduction of the second half of the groups (_range:
 * two-stage calls only).  _range transforms the already reduced partial stacks g_begin <= g < g_end of the reduce buffer
 * and adds them to the linear / phase stacks (ts_pws1f_lib.c:885-906); g_begin == 0 starts from zero, and ranges must
 * be given in increasing order so that the sums keep the reference's trace order.  _tail applies the weight, both inverse
 * transforms and the epilogue (ts_pws1f_lib.c:226-241).  tspws_hip_stack_finish == _range(0, Kmax) + _tail. */
int  tspws_hip_stack_finish_range(tspws_hip_plan *plan, const t_tsPWS *p, size_t mtr_global,
                                  unsigned g_begin, unsigned g_end, void *stream);
int  tspws_hip_stack_finish_tail(tspws_hip_plan *plan, const t_tsPWS *p, size_t mtr_global,
                                 float *d_ls, float *d_tsPWS, void *stream);

/* Single-GPU convenience: _local + _finish in one call; on return all work is ordered on `stream`. */
int  tspws_hip_stack(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, size_t mtr,
                     float *d_ls, float *d_tsPWS, void *stream);
/* B ensembles of the same trace length, one stack each.  Ensemble b is the traces [h_first[b], h_first[b+1]) of d_sigall (h_first has
 * B + 1 non-decreasing host entries, h_first[0] may be > 0).  Row b of d_ls / d_tsPWS ([B][max] floats) receives what
 * tspws_hip_stack(plan, p, d_sigall + h_first[b] * ld, ld, h_first[b+1] - h_first[b], ...) would write, to the parity tolerance (relerr
 * 2e-6; a call with B = 1 IS that call).  Every ensemble follows the single call's rules: two-stage iff 0 < Kmax <= M_b
 * (tspws_is_two_stage), weights with K = M = M_b (single-stage) or (Kmax, M_b), ls divided by M_b; a batch may mix both kinds.  An empty
 * ensemble (M_b = 0) gives zero rows.  Fold and mean removal stay with the caller (tspws_hip_fold / tspws_hip_remove_mean on the whole
 * array).  The single-stage ensembles go through ONE many-trace pass when their total trace count takes that path (each ensemble starts a
 * fresh 64-trace block), the two-stage ensembles through one streaming pass and one few-row finish.  Every scratch block that grows with
 * the ensembles stays within TSPWS_PART_MB (ensembles are processed in rounds).  NULL pointers, decreasing offsets or ld < max return TSPWS_E_ARG before any device work; B = 0
 * returns 0 and does nothing.  The call waits for `stream`: on return the outputs are complete. */
int  tspws_hip_stack_batch(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, const size_t *h_first, unsigned B,
                           float *d_ls, float *d_tsPWS, void *stream);
/* How the ensembles of the plan's last tspws_hip_stack_batch call with B > 0 were stacked (all zero before the first one). */
typedef struct {
	unsigned single_pass;    /* single-stage ensembles stacked by the shared many-trace pass                               */
	unsigned two_stage_pass; /* two-stage ensembles stacked by the shared streaming pass and few-row finish                */
	unsigned looped;         /* ensembles stacked by one tspws_hip_stack each (below the many-trace rule / alone of their kind) */
	unsigned empty;          /* ensembles without traces (zero rows)                                                      */
	unsigned rounds;         /* rounds of the two shared passes (scratch budget; a round never splits an ensemble)        */
	unsigned pass_batches;   /* batches of the many-trace pass (an ensemble may straddle two)                             */
} tspws_hip_batch_stats;
int  tspws_hip_stack_batch_stats(const tspws_hip_plan *plan, tspws_hip_batch_stats *stats);
/* tspws_hip_stack_batch with a band-limited finish: the ensembles, stage rule, weights and rounds are tspws_hip_stack_batch's (single- and
 * two-stage ensembles may be mixed); with (OUT_b, ST_b) the weighted set and the linear stack that call inverts and M_b the trace count,
 * the outputs are [B][R][max] floats (tspws_hip_inverse_bands' definitions)
 *   ts[b][r] = (float) X_r(OUT_b)        ts_env[b][r] = (float) E_r(OUT_b)
 *   ls[b][r] = (float) X_r(ST_b) / (float) M_b   ls_env[b][r] = (float) E_r(ST_b) / (float) M_b   (the reference's float division, :233-241)
 * written by the combining kernel itself (no FP64 row in memory).  Each set is read once, whatever R.  d_ls_env and d_ts_env are both NULL
 * (no quadrature work at all; ls / ts have the same bits either way) or both given.  Empty ensembles and empty bands give zero rows; the
 * band [0, S) gives tspws_hip_stack_batch's rows to the parity tolerance (relerr 2e-6).  Ensembles that tspws_hip_stack_batch hands to
 * one tspws_hip_stack each get their sets from tspws_hip_stacks_float, or tspws_hip_partial_stacks + tspws_hip_stacks_double, and
 * tspws_hip_weight.  Refusals (TSPWS_E_ARG, "stack_batch_bands: ..." before any device work, outputs untouched): tspws_hip_stack_batch's,
 * tspws_hip_inverse_bands', and exactly one envelope pointer; B = 0 or R = 0 returns 0 and does nothing.  The call waits for `stream`. */
int  tspws_hip_stack_batch_bands(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, const size_t *h_first, unsigned B,
                                 const tspws_band *h_bands, unsigned R, float *d_ls, float *d_tsPWS, float *d_ls_env, float *d_tsPWS_env,
                                 void *stream);
/* The plan's last tspws_hip_stack_batch_bands call with B > 0 and R > 0 (all zero before the first one). */
typedef struct {
	tspws_hip_batch_stats batch; /* tspws_hip_stack_batch's counters                                                         */
	unsigned finish_batches;     /* batches of sets of the band finish (scale rows within TSPWS_PART_MB)                      */
	unsigned scales;             /* scales inside at least one band: work items of the inverse, slot rows per set             */
	unsigned quadrature;         /* 1: the quadrature ran (envelopes asked for)                                               */
} tspws_hip_stack_bands_stats;
int  tspws_hip_stack_batch_bands_stats(const tspws_hip_plan *plan, tspws_hip_stack_bands_stats *stats);
/* Optional timing inside tspws_hip_stack: HIP events on `stream` at the start of the call, after its streaming stage (the
 * partial-stack launches) and at its end, for up to max_calls calls.  _read synchronises the device and returns the per-call
 * durations in ms (either array may be NULL; *ncalls = calls recorded); _end returns the mean of the streaming stage and
 * resets the recorder. */
int  tspws_hip_profile_begin(tspws_hip_plan *plan, size_t max_calls);
int  tspws_hip_profile_read(tspws_hip_plan *plan, double *stage_ms, double *call_ms, size_t cap, size_t *ncalls);
int  tspws_hip_profile_end(tspws_hip_plan *plan, double *mean_ms, size_t *ncalls);
/* Number of streaming-kernel (k_partial) launches the last partial-stack / stack_local call issued: the traces are walked a
 * few groups at a time so that every launch puts one workgroup on every CU. */
int  tspws_hip_stream_launches(const tspws_hip_plan *plan);

/* ---- scale-sharded finish stage (multi-GPU; no counterpart in the reference) ---------------------------------------------
 * After the all-reduce every rank holds the same Kmax partial stacks.  The transforms, the weighting and the inverse are
 * separable by scale and the reconstruction is a SUM over scales: rank r finishes only its share of the scales and the
 * ranks add their partial reconstructions (2 * max doubles) before tspws_hip_epilogue.
 *   _finish_shard : work-balanced, contiguous share [*s_begin, *s_end) of the scales (whole decimation octaves, possibly
 *                   empty) of `rank` in `world`; returns 1 (not an error) when the plan / parameters have no sharded finish
 *                   (single-stage calls, debug kernels, >= 64 groups): finish with tspws_hip_stack_finish then.
 *   _finish_scales: transforms + stacks + weights + inverse of those scales from the reduced partial stacks
 *                   (tspws_hip_reduce_buffer); d_x2 receives [ICWT(OUT) | ICWT(ST)] restricted to them, 2 * max doubles. */
int  tspws_hip_finish_shard(const tspws_hip_plan *plan, const t_tsPWS *p, size_t mtr_global, unsigned rank, unsigned world,
                            unsigned *s_begin, unsigned *s_end);
int  tspws_hip_stack_finish_scales(tspws_hip_plan *plan, const t_tsPWS *p, size_t mtr_global, unsigned s_begin, unsigned s_end,
                                   double *d_x2, void *stream);

/* ---- jackknife (two-stage only, like the reference) ------------------------------------- */
/* Host: deletion masks sel[C][mtr] (1 = kept) from start times.  JackknifePlans, :385-430.
 * Returns 0, 1 for NULL arguments, -2 when time[0]==0 (no start times). */
int  tspws_jackknife_plan(char *sel, const time_t *time, size_t mtr, unsigned d, unsigned n, unsigned C);
/* Device: all C replicas from ONE pass over the traces.  TwoStage_jackknife_float, :719-831.
 * d_ls_out / d_ts_out are [C][max] floats; h_mtr_out receives the C replica sizes. */
int  tspws_hip_jackknife(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld,
                         size_t mtr, const char *h_sel, unsigned C,
                         float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out, void *stream);

/* The two-stage stack AND its C jackknife replicas from ONE pass over the device-resident traces (the reference walks them
 * 1 + C times, :216 and :758-772): same outputs as tspws_hip_stack followed by tspws_hip_jackknife, except that the stack's
 * groups are summed class by class (last-bit differences in the FP64 partial stacks).  Falls back to tspws_hip_stack for
 * single-stage parameters or C == 0.  h_mtr_out is filled on return; the device outputs are ordered on `stream` like tspws_hip_stack's
 * (the call waits for the stream itself only when it had to upload the tables of a selection it has not seen in its last call). */
int  tspws_hip_stack_jackknife(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, size_t mtr,
                               float *d_ls, float *d_tsPWS, const char *h_sel, unsigned C,
                               float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out, void *stream);

/* Trace-sharded jackknife (one shard per GPU; the reference has no counterpart -- its replicas, :735-813, walk one host
 * array).  h_sel is the selection over the WHOLE ensemble, [C][mtr_global]; a trace's group in a replica is its rank among
 * all selected traces (:766), so every shard evaluates the signatures globally and sums only its own traces.
 *   _buffer : device rows [C * Kmax][max] doubles (row c * Kmax + g = group g of replica c), *nd = their count.
 *   _local  : ONE pass over the shard fills those rows AND the rows of the plain two-stage groups
 *             (tspws_hip_reduce_buffer) with the shard's sums; an empty shard gives zeros.  The caller adds the shards
 *             (all-reduce, or a reduce of each replica's rows to the rank that owns it).
 *   _finish : replicas [c_begin, c_end) from the (reduced) rows; outputs go to rows c_begin.. of the [C][max] arrays,
 *             replica sizes to h_mtr_out[c_begin..]. */
int  tspws_hip_jackknife_buffer(tspws_hip_plan *plan, const t_tsPWS *p, unsigned C, double **d_buf, size_t *nd);
int  tspws_hip_jackknife_local(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, size_t mtr_local,
                               size_t first, size_t mtr_global, const char *h_sel, unsigned C, void *stream);
int  tspws_hip_jackknife_finish(tspws_hip_plan *plan, const t_tsPWS *p, size_t mtr_global, const char *h_sel, unsigned C,
                                unsigned c_begin, unsigned c_end, float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out,
                                void *stream);

/* ---- single-stage jackknife (an extension: the reference's tspws_jackknife_float, :711-716, is an empty stub) ---------------
 * Host: classes of a selection sel[C][mtr] (1 = kept): the traces whose selection columns are identical, numbered in order of first
 * appearance.  class_of_trace receives mtr class numbers, *ncls the class count; kept (may be NULL; room for C * mtr bytes at most)
 * receives [C][*ncls] bytes, 1 = replica c keeps class k.  A jackknife selection has n or n + 1 classes (day-of-year bins). */
int  tspws_selection_classes(const char *sel, unsigned C, size_t mtr, unsigned *class_of_trace, char *kept, unsigned *ncls);
/* Device: the C replicas of a SINGLE-stage parameter set (two-stage: TSPWS_E_ARG).  Replica c is the single-stage resampling body
 * (tspws_subsmpl_float, :501-610) on mask row c with K = M = K_c (its selected traces): tsPWS_out[c] = (float) Re_rec(weight(ST_c, PS_c));
 * ls_out[c] = (float)((sum of the selected traces, FP64) * (1 / K_c)); h_mtr_out[c] = K_c; K_c = 0 gives zero rows.  Every trace is
 * transformed once into per-class stacks, the replicas are sums of classes.  Same arguments as tspws_hip_jackknife; returns with its
 * outputs complete. */
int  tspws_hip_jackknife_single(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, size_t mtr,
                                const char *h_sel, unsigned C, float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out, void *stream);

/* The single-stage jackknife of B ensembles of one trace array in ONE call.  Ensemble b is the traces [h_first[b], h_first[b+1]) of d_sigall
 * (the rules of tspws_hip_stack_batch: B + 1 non-decreasing host entries, h_first[0] may be > 0).  h_sel is [C][T] bytes (1 = kept), T =
 * h_first[B] - h_first[0]: column i - h_first[0] belongs to trace i, every ensemble has the same C; the caller builds each ensemble's columns
 * with tspws_jackknife_plan on that ensemble's own start times (any 0/1 matrix is accepted).  The replica block [b][C][max] of d_ls_out /
 * d_ts_out and h_mtr_out[b][C] receive what tspws_hip_jackknife_single gives for ensemble b alone with its columns (K_c = 0: zero rows, count
 * 0), row b of d_ls / d_tsPWS ([B][max]; both NULL: not wanted) what tspws_hip_stack_batch writes for it (weights with K = M = M_b, ls by
 * a float division by M_b), to the parity tolerance (relerr 2e-6).  An empty ensemble gives zero rows and zero counts.  Single-stage parameter
 * sets only: tspws_is_two_stage for any ensemble returns TSPWS_E_ARG (tspws_hip_jackknife is the two-stage route), and so do NULL plan / p /
 * h_first / h_sel / replica outputs / h_mtr_out, exactly one of d_ls / d_tsPWS NULL, decreasing offsets, ld < max and more than 65535 classes
 * (distinct selection columns) in one ensemble -- all before any device work.  B == 0 or C == 0 returns 0 and does nothing.  Fold and mean
 * removal stay with the caller.  When the total trace count takes the many-trace path, every (ensemble, class) starts a fresh 64-trace block
 * of ONE shared pass in which every trace is transformed once, and every replica is a sum of its ensemble's class planes; otherwise the call
 * is one tspws_hip_stack + tspws_hip_jackknife_single per ensemble.  Every scratch block that grows with the ensembles stays within
 * TSPWS_PART_MB (rounds of whole ensembles; one ensemble alone may exceed it).  The call uploads host tables and waits for `stream`: on
 * return the outputs are complete. */
int  tspws_hip_jackknife_batch(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, const size_t *h_first, unsigned B,
                               const char *h_sel, unsigned C, float *d_ls, float *d_tsPWS, float *d_ls_out, float *d_ts_out,
                               unsigned *h_mtr_out, void *stream);
/* How the plan's last tspws_hip_jackknife_batch call with B > 0 and C > 0 went (all zero before the first one). */
typedef struct {
	unsigned shared;       /* ensembles that went through the shared many-trace pass                            */
	unsigned looped;       /* ensembles finished by one tspws_hip_stack + tspws_hip_jackknife_single each       */
	unsigned empty;        /* ensembles without traces (zero rows, zero counts)                                 */
	unsigned rounds;       /* rounds forced by the scratch budget (a round never splits an ensemble)            */
	unsigned pass_batches; /* batches of the many-trace pass (a class may straddle two)                         */
	unsigned classes;      /* (ensemble, class) segments in total                                               */
} tspws_hip_jk_batch_stats;
int  tspws_hip_jackknife_batch_stats(const tspws_hip_plan *plan, tspws_hip_jk_batch_stats *stats);

/* The TWO-stage jackknife (TwoStage_jackknife_float, :719-831) of B ensembles of one trace array in ONE call.  Arguments as
 * tspws_hip_jackknife_batch: h_first has B + 1 non-decreasing host entries (h_first[0] may be > 0), ld > max is allowed, h_sel is [C][T]
 * bytes (1 = kept; any 0/1 matrix), T = h_first[B] - h_first[0].  The replica block [b][C][max] of d_ls_out / d_ts_out and h_mtr_out[b][C]
 * receive what tspws_hip_jackknife gives for ensemble b alone with its columns: the group of a selected trace is floor(k Kmax / K_c), k its
 * rank among the selected traces (:766); tsPWS_out = (float) Re_rec(weight(ST_c, PS_c; K = Kmax, M = K_c)); ls_out = (float)((sum of the
 * groups' partial stacks) * (1 / K_c)), formed in the time domain (:799-811); h_mtr_out = K_c.  A replica with 0 < K_c < Kmax has empty
 * groups, whose rows count as zero (as in the reference); K_c = 0 gives zero rows and count 0 (the batch calls' choice: the single call
 * divides by zero there).  Row b of d_ls / d_tsPWS ([B][max]; both NULL: not wanted) is what tspws_hip_stack_batch writes for the ensemble
 * (weights with (Kmax, M_b), ls by a float division by M_b).  All to the parity tolerance (relerr 2e-6).  An empty ensemble gives zero
 * rows and zero counts.  Two-stage parameter sets only: a non-empty ensemble that is not two-stage by tspws_is_two_stage (Kmax == 0 or
 * Kmax > M_b) returns TSPWS_E_ARG ("single-stage": tspws_hip_jackknife_batch is that route), and so do NULL plan / p / h_first / h_sel /
 * replica outputs / h_mtr_out, exactly one of d_ls / d_tsPWS NULL, decreasing offsets and ld < max -- all before any device work, outputs
 * untouched.  B == 0 or C == 0 returns 0 and does nothing.  Fold and mean removal stay with the caller.
 * With ONE non-empty ensemble the call IS tspws_hip_stack_jackknife for it (tspws_hip_jackknife without the main rows), bit for bit.  With
 * two or more, one streaming kernel walks every ensemble's traces once: a workgroup owns one (ensemble, tile of <= 16 columns, 1024 samples),
 * keeps a running FP64 sum per column in registers and stores the Kmax partial-stack rows of every column (replicas and, as the last column
 * of the last tile, the plain stack) -- no atomics, every row written by one workgroup; then one forward launch over all rows of the round,
 * one accumulation, the weights with each column's trace count, the replicas' linear stacks, one batched inverse and the float epilogue.
 * Every scratch block that grows with the ensembles stays within TSPWS_PART_MB (rounds of whole ensembles; one ensemble alone may exceed
 * it).  The call uploads one table block per round and waits for `stream`: on return the outputs are complete. */
int  tspws_hip_jackknife_batch_two_stage(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, const size_t *h_first,
                                         unsigned B, const char *h_sel, unsigned C, float *d_ls, float *d_tsPWS, float *d_ls_out,
                                         float *d_ts_out, unsigned *h_mtr_out, void *stream);
/* How the plan's last tspws_hip_jackknife_batch_two_stage call with B > 0 and C > 0 went (all zero before the first one). */
typedef struct {
	unsigned shared;       /* ensembles that went through the shared walk                                       */
	unsigned looped;       /* 1: the only non-empty ensemble went through tspws_hip_stack_jackknife / _jackknife */
	unsigned empty;        /* ensembles without traces (zero rows, zero counts)                                 */
	unsigned rounds;       /* rounds forced by the scratch budget (a round never splits an ensemble)            */
	unsigned tiles;        /* column tiles (of <= 16 columns) per ensemble                                      */
	unsigned rows;         /* partial-stack rows transformed in total                                           */
} tspws_hip_jk_batch2_stats;
int  tspws_hip_jackknife_batch_two_stage_stats(const tspws_hip_plan *plan, tspws_hip_jk_batch2_stats *stats);

/* ---- random subsampling ---------------------------------------------------------------------- */
/* Host: keep K of J traces at random with libc rand(), flipping whichever symbol is rarer.
 * SubsamplingPlan, ts_pws1f_lib.c:355-383 (same rand() call order, so the same masks from the same state). */
int  tspws_subsampling_plan(char *sel, size_t J, size_t K);
/* M random subsamples of K = ceil(mtr * p->subsmpl_p) traces; d_ls_out / d_ts_out are [M][max] floats.
 * Single-stage: tspws_subsmpl_float (:501-610); two-stage: TwoStage_subsmpl_float (:612-709). */
int  tspws_hip_subsample(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, size_t mtr, unsigned M,
                         float *d_ls_out, float *d_ts_out, void *stream);
/* The same with the M masks given (h_sel[M][mtr], 1 = kept: M calls of tspws_subsampling_plan with K = ceil(mtr * subsmpl_p)).
 * tspws_main draws them BEFORE its first HIP call: the initialisation of the HIP runtime inside a process's first call consumes
 * libc rand() values, and the masks are to come from the state the caller seeded, as in the reference. */
int  tspws_hip_subsample_sel(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, size_t mtr, unsigned M,
                             const char *h_sel, float *d_ls_out, float *d_ts_out, void *stream);

/* Host: the masks of a batch, sel[M][T] (1 = kept), T = first[B] - first[0]: for b = 0 .. B-1 in order, for m = 0 .. M-1 in order,
 * tspws_subsampling_plan(the columns of ensemble b in row m, M_b, ceil(M_b * prob)) -- the rand() call order of a loop of
 * tspws_hip_subsample over the ensembles.  Empty ensembles draw nothing.  Returns 0; 1 for NULL arguments or decreasing offsets (nothing
 * written, nothing drawn); 2 where prob asks for more than M_b traces (prob > 1). */
int  tspws_subsampling_plan_batch(char *sel, const size_t *first, unsigned B, unsigned M, double prob);
/* M random subsamples of each of B ensembles of one trace array in ONE call, the masks given.  Ensemble b = the traces [h_first[b],
 * h_first[b+1]) of d_sigall (the rules of tspws_hip_stack_batch: B + 1 non-decreasing host offsets, h_first[0] may be > 0, ld >= max);
 * h_sel is [M][T] bytes (1 = kept; any 0/1 matrix), T = h_first[B] - h_first[0], column i - h_first[0] for trace i.  K_{b,m} = the ones of
 * row m inside ensemble b = h_mtr_out[b][m]; with masks from tspws_subsampling_plan_batch K_{b,m} = ceil(M_b * subsmpl_p) for every m, and
 * block [b][M][max] of d_ls_out / d_ts_out then is what tspws_hip_subsample_sel gives for ensemble b alone with its columns, to the parity
 * tolerance (relerr 2e-6).  Every ensemble follows the single call's rule on its own size -- two-stage iff 0 < Kmax <= M_b (by M_b, not by
 * K) -- and a batch may mix both kinds:
 *   single-stage (tspws_subsmpl_float, :501-610): tsPWS_out = (float) Re_rec(weight(ST, PS)) of the kept traces with K = M = K_{b,m}, the
 *     mode chosen per row (a K = 1 row takes the K = 1 rule); ls_out = the FLOAT accumulator over the kept traces in trace order (:538-542)
 *     times (float)(1. / K_{b,m}) (:579-583);
 *   two-stage (TwoStage_subsmpl_float, :612-709): the group of a kept trace is floor(k Kmax / K_{b,m}), k its rank among the kept traces;
 *     weights with (Kmax, K_{b,m}); ls_out = (float)((the groups' FP64 sum) * (1 / K_{b,m})); empty groups (K_{b,m} < Kmax) count as zero rows.
 * K_{b,m} = 0 gives zero rows and count 0 (the batch calls' choice); an empty ensemble gives zero rows and zero counts.  B == 0 or M == 0
 * returns 0 and does nothing.  NULL plan / p / h_first / h_sel / outputs / h_mtr_out, NULL traces with T > 0, decreasing offsets and
 * ld < max return TSPWS_E_ARG ("subsample_batch: ...") before any device work, outputs untouched; the checks that need no plan come first.
 * Fold and mean removal stay with the caller.
 * With ONE non-empty ensemble the call IS tspws_hip_subsample_sel for it, bit for bit, when every row has K = ceil(M_b subsmpl_p) (a
 * two-stage ensemble: whenever no row is empty).  Otherwise, in rounds of whole ensembles: the single-stage ensembles' traces are transformed once (one
 * forward launch sequence per stretch of contiguous traces), ONE segmented masked accumulation (coefficient tile x group of 8 masks x
 * ensemble; the 8 mask bits of a trace in one byte) leaves every row's ST / PS planes, written once, ONE kernel forms the float-accumulator
 * linear stacks, then the weights with each row's K, the batched inverses and the float epilogue scattered to [b][m]; the two-stage
 * ensembles go through the shared walk of tspws_hip_jackknife_batch_two_stage without main rows.  Nothing is atomic, every sum has a fixed
 * order: a repeated call is bit-identical.  Every scratch block that grows with the batch stays within TSPWS_PART_MB (a round never splits
 * an ensemble; one ensemble alone may exceed it).  The call uploads its tables and waits for `stream`: on return the outputs are complete. */
int  tspws_hip_subsample_batch_sel(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, const size_t *h_first, unsigned B,
                                   unsigned M, const char *h_sel, float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out, void *stream);
/* The same with the masks drawn by tspws_subsampling_plan_batch(p->subsmpl_p) BEFORE the call's first device call (after its refusals: a
 * refused call draws nothing). */
int  tspws_hip_subsample_batch(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, const size_t *h_first, unsigned B,
                               unsigned M, float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out, void *stream);
/* How the plan's last tspws_hip_subsample_batch[_sel] call with B > 0 and M > 0 went (all zero before the first one). */
typedef struct {
	unsigned single_shared;    /* single-stage ensembles that went through the segmented accumulation               */
	unsigned two_stage_shared; /* two-stage ensembles that went through the shared walk                              */
	unsigned looped;           /* 1: the only non-empty ensemble went through tspws_hip_subsample_sel                */
	unsigned empty;            /* ensembles without traces (zero rows, zero counts)                                  */
	unsigned rounds;           /* rounds of single-stage ensembles + rounds of the walk (0 when looped)              */
	unsigned rows;             /* mask rows finished: M per non-empty ensemble                                       */
} tspws_hip_sub_batch_stats;
int  tspws_hip_subsample_batch_stats(const tspws_hip_plan *plan, tspws_hip_sub_batch_stats *stats);

/* ---- bootstrap ------------------------------------------------------------------------------- */
/* Host: one bootstrap draw of J traces with replacement, cnt[i] = how often trace i was drawn: J counts are cleared, then J draws
 * i = (size_t)(rand() * ((double)J / ((double)RAND_MAX + 1.0))), cnt[i]++ (a draw that lands on a count of 255 is drawn again).  Returns 0;
 * 1 for a NULL argument (nothing drawn).  J == 0 draws nothing. */
int  tspws_bootstrap_plan(unsigned char *cnt, size_t J);
/* Host: the counts of a batch, cnt[M][T], T = first[B] - first[0]: for b = 0 .. B-1 in order, for m = 0 .. M-1 in order,
 * tspws_bootstrap_plan(the columns of ensemble b in row m, M_b) -- the rand() call order of a loop over the ensembles.  Empty ensembles
 * draw nothing.  Returns 0; 1 for NULL arguments or decreasing offsets (nothing written, nothing drawn). */
int  tspws_bootstrap_plan_batch(unsigned char *cnt, const size_t *first, unsigned B, unsigned M);
/* M bootstrap replicas of each of B single-stage ensembles of one trace array in ONE call, the counts given.  Ensemble b = the traces
 * [h_first[b], h_first[b+1]) of d_sigall (the rules of tspws_hip_stack_batch: B + 1 non-decreasing host offsets, h_first[0] may be > 0,
 * ld >= max); h_cnt is [M][T] unsigned bytes, T = h_first[B] - h_first[0], column i - h_first[0] for trace i (the layout of h_sel in
 * tspws_hip_subsample_batch_sel): cnt[m][i] = how often trace i enters replica m.  Replica (b, m) is the single-stage resampling body
 * (tspws_subsmpl_float, :501-610) with an all-ones mask on the EXPANDED ensemble -- the traces of ensemble b in trace order, trace i
 * repeated cnt[m][i] times -- which is never formed.  With K = K_{b,m} = the counts of row m inside ensemble b = h_mtr_out[b][m]:
 *   ST = sum_i cnt_i Y_i, PS = sum_i cnt_i Y_i / |Y_i| (the phasor rule of the stacks), the copies added one after the other in trace order:
 *     repeated addition, not a multiplication by the count, so the order of operations is that of the expanded ensemble, and a 0/1 count
 *     row runs exactly the arithmetic of tspws_hip_subsample_batch_sel on that row as a mask;
 *   tsPWS_out[b][m] = (float) Re_rec(weight(ST, PS)) with K = M = K_{b,m}, the mode chosen per row (a K = 1 row takes the K = 1 rule);
 *   ls_out[b][m] = the FLOAT accumulator over the expanded ensemble, acc = (float)((double)acc + (double)x) once per copy in trace order
 *     (:538-542), times (float)(1. / K_{b,m}) (:579-583).
 * K_{b,m} = 0 gives zero rows and count 0; an empty ensemble gives zero rows and zero counts.  d_ls_out / d_ts_out are [B][M][max] floats on
 * the device, h_mtr_out [B][M] on the host.  d_stats is NULL (not wanted) or [B][4][max] floats on the device: per sample, over the
 * replicas of ensemble b with K > 0 (n of them), the mean of ls_out, its standard error, the mean of ts_out, its standard error -- two FP64
 * passes in replica order over the float rows: mean = (sum v) / n, error = sqrt(sum (v - mean)^2 / (n - 1)), the bootstrap standard error;
 * n <= 1 gives error 0, n = 0 a zero mean.  B == 0 or M == 0 returns 0 and does nothing.  NULL plan / p / h_first / h_cnt / outputs /
 * h_mtr_out, NULL traces with T > 0, decreasing offsets, ld < max and a non-empty ensemble that is two-stage (0 < Kmax <= M_b: in the
 * expanded ensemble a repeated trace can straddle the borders of the groups floor(k Kmax / K), which needs a walk of its own; the message
 * says "two-stage") return TSPWS_E_ARG ("bootstrap_batch: ...") before any device work, outputs untouched; the checks that need no plan
 * come first.  Fold and mean removal stay with the caller.
 * In rounds of whole ensembles: the traces are transformed once (one forward launch sequence per stretch of contiguous traces), ONE
 * segmented counted accumulation (coefficient tile x group of 8 replicas x ensemble; the 8 counts of a trace in one aligned 8-byte word)
 * leaves every row's ST / PS planes, written once, ONE kernel forms the float-accumulator linear stacks, then the weights with each row's
 * K, the batched inverses, the float epilogue scattered to [b][m] and ONE kernel per round for the statistics.  Nothing is atomic, every
 * sum has a fixed order: a repeated call is bit-identical.  Every scratch block that grows with the batch stays within TSPWS_PART_MB (a
 * round never splits an ensemble; one ensemble alone may exceed it).  The call uploads its tables and waits for `stream`: on return the
 * outputs are complete. */
int  tspws_hip_bootstrap_batch_cnt(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, const size_t *h_first, unsigned B,
                                   unsigned M, const unsigned char *h_cnt, float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out, float *d_stats,
                                   void *stream);
/* The same with the counts drawn by tspws_bootstrap_plan_batch BEFORE the call's first device call (after its refusals: a refused call
 * draws nothing; the reason for the order stands above tspws_hip_subsample_sel).  Every K_{b,m} then is M_b. */
int  tspws_hip_bootstrap_batch(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, const size_t *h_first, unsigned B,
                               unsigned M, float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out, float *d_stats, void *stream);
/* How the plan's last tspws_hip_bootstrap_batch[_cnt] call with B > 0 and M > 0 went (all zero before the first one). */
typedef struct {
	unsigned shared;    /* ensembles that went through the segmented counted accumulation   */
	unsigned empty;     /* ensembles without traces (zero rows, zero counts)                */
	unsigned rounds;    /* rounds forced by the scratch budget (a round never splits an ensemble) */
	unsigned rows;      /* replica rows finished: M per non-empty ensemble                  */
	unsigned max_count; /* the largest count of the batch                                   */
} tspws_hip_boot_batch_stats;
int  tspws_hip_bootstrap_batch_stats(const tspws_hip_plan *plan, tspws_hip_boot_batch_stats *stats);

/* ---- real-weighted stacks ------------------------------------------------------------------------- */
/* M real-weighted stacks of each of B single-stage ensembles of one trace array in ONE call: the soft counterpart of a mask row or a count
 * row (days weighted by 1 / energy, by similarity^p, by an SNR; several weightings side by side).  Ensembles, offsets, ld and the layout of
 * h_w ([M][T] doubles, T = h_first[B] - h_first[0], column i - h_first[0] for trace i) are those of tspws_hip_bootstrap_batch_cnt.  The
 * reference's linear stack has a hook for this (tspws_stacks_float's w, ts_pws1f_lib.c:485-490) that nothing passes and that leaves the
 * phase stack and the normalisers unweighted; scaling a copy of the traces cannot say it either, since w Y / |w Y| = Y / |Y|.  For row m of
 * ensemble b, with w_i = h_w[m][i - h_first[0]] >= 0:
 *   a trace with w_i == 0 takes no part at all: its coefficients, phasors and samples never reach a sum, exactly like a masked-out trace;
 *   n+ = the traces with w_i > 0 = h_mtr_out[b][m] (tspws_hip_replica_bands runs on the rows as on the other calls' rows);
 *   W = sum w_i and Q = sum w_i^2, in FP64, on the host, in trace order; Keff = W W / Q, the effective number of traces, to h_keff[b][m]
 *     (h_keff: NULL or [B][M] host doubles; 0 when n+ == 0).  For 0/1 rows W = Keff = K exactly;
 *   ST = sum w_i Y_i, PS = sum w_i Y_i / |Y_i| (the phasor rule of the stacks), in trace order, each trace summed over its splits first, one
 *     fused multiply-add per component (w in {0, 1}: the bits of an addition);
 *   the coherence is c = |PS| / W.  For random phases E |PS|^2 = Q, so the bias of c^2 is Q / W^2 = 1 / Keff, and with OUT = the weighted
 *     coefficient:  unbiased (wu == 2 && unbiased && n+ != 1): OUT = ST (Keff c^2 - 1) / (Keff - 1) / W;  biased, wu == 2: ST |PS|^2 / (W^2 W);
 *     wu == 1: ST |PS| / (W W);  any other wu: ST (|PS| / W)^wu / W.  n+ == 1 takes the K = 1 rule (:972), and so does a row whose Keff is exactly 1 in FP64 (one weight carries
 *     the row: Keff - 1 == 0).  A Keff just above 1 keeps the formula, which then amplifies the rounding of c^2 by 1 / (Keff - 1): a row that
 *     one trace dominates has no bias to average away -- read h_keff.  The expressions are those of the
 *     other batched calls with (W, Keff) in place of (K, K): a 0/1 row gives the bits of tspws_hip_subsample_batch_sel on that row as a mask;
 *   tsPWS_out[b][m] = (float) Re_rec(OUT);
 *   ls_out[b][m] = the FLOAT accumulator of the resampling body (:538-542) with a weighted addend, acc = (float)((double)acc + w_i *
 *     (double)x_i[n]) (the product rounded on its own) over the participating traces in trace order, times (float)(1. / W) (:579-583).
 * Multiplying a row by a power of two leaves its outputs bit for bit (short of overflow and underflow).  n+ == 0 gives zero rows, count 0
 * and Keff 0; an empty ensemble gives the same.  d_ls_out / d_ts_out are [B][M][max] floats on the device, h_mtr_out [B][M] on the host.
 * B == 0 or M == 0 returns 0 and does nothing.  NULL plan / p / h_first / h_w / outputs / h_mtr_out, NULL traces with T > 0, decreasing
 * offsets, ld < max, more than 2^32 - 16 traces in an ensemble, a weight inside an ensemble that is NaN, infinite or negative (the message
 * says "weight"), a row of an ensemble whose W or Q is not finite or whose Q underflows to zero, and a non-empty two-stage ensemble
 * (0 < Kmax <= M_b; the message says "two-stage": with real weights the groups floor(k Kmax / K) have no meaning -- by design, not a gap)
 * return TSPWS_E_ARG ("weighted_stack_batch: ...") before any device work, outputs untouched; the checks that need no plan come first.
 * Fold and mean removal stay with the caller.
 * In rounds of whole ensembles: the traces are transformed once (one forward launch sequence per stretch of contiguous traces), ONE
 * segmented weighted accumulation (coefficient tile x group of 8 rows x ensemble; the 8 weights of a trace in one aligned 64-byte block,
 * read through a wave-uniform address; a zero weight is a wave-uniform skip) leaves every row's ST / PS planes, written once, ONE kernel
 * forms the float-accumulator linear stacks, then the weights with each row's (n+, W, Keff), the batched inverses and the float epilogue
 * scattered to [b][m].  Nothing is atomic, every sum has a fixed order: a repeated call is bit-identical.  Every scratch block that grows
 * with the batch stays within TSPWS_PART_MB (a round never splits an ensemble; one ensemble alone may exceed it).  The call uploads its
 * tables and waits for `stream`: on return the outputs are complete. */
int  tspws_hip_weighted_stack_batch(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, const size_t *h_first, unsigned B,
                                    unsigned M, const double *h_w, float *d_ls_out, float *d_ts_out, unsigned *h_mtr_out, double *h_keff,
                                    void *stream);
/* How the plan's last tspws_hip_weighted_stack_batch call with B > 0 and M > 0 went (all zero before the first one). */
typedef struct {
	unsigned shared;    /* ensembles that went through the segmented weighted accumulation  */
	unsigned empty;     /* ensembles without traces (zero rows, zero counts)                */
	unsigned rounds;    /* rounds forced by the scratch budget (a round never splits an ensemble) */
	unsigned rows;      /* weight rows finished: M per non-empty ensemble                   */
} tspws_hip_weighted_batch_stats;
int  tspws_hip_weighted_stack_batch_stats(const tspws_hip_plan *plan, tspws_hip_weighted_batch_stats *stats);
/* Host: one weight row from one plane of tspws_hip_trace_scores.  score is [T] doubles, T = first[B] - first[0]; w receives [T] doubles
 * (one row of h_w).
 *   rule 0 (a similarity plane): w = score > 0 ? pow(score, a) : 0 -- NaN and non-positive scores give 0.
 *   rule 1 (the energy plane): w = 1 / score for a finite score > 0, else 0; then divided by the largest w of the ensemble, so that a
 *           row's W cannot overflow; an ensemble without a positive finite score gets zeros.  a is ignored.
 * Returns 0; 1 for NULL w / score / first or decreasing offsets (nothing written); 2 for an unknown rule, or a NaN a under rule 0 (nothing
 * written). */
int  tspws_weights_from_scores(double *w, const double *score, const size_t *first, unsigned B, int rule, double a);

/* ---- percentile bands of replicas ---------------------------------------------------------------- */
/* Per sample, Q quantiles over the replicas of each of B ensembles.  d_rows is [B][M][ld] floats on the plan's device (what the batched
 * resampling calls write as d_ls_out / d_ts_out: ld = max), h_mtr NULL or [B][M] host counts (their h_mtr_out): replica (b, m) takes part
 * iff h_mtr == NULL or h_mtr[b][m] > 0.  d_bands is [B][Q][N] floats, N = the plan's trace length.
 * For ensemble b let n be the replicas that take part and x_(0) <= ... <= x_(n-1) their values at sample s, in the order of the usual
 * order-preserving integer key of a float's bits (negative values: all bits flipped, the others: the sign bit set; infinities sort at the
 * ends, NaNs by their bit pattern -- inputs are meant to be finite, others neither fault nor hang and follow the same arithmetic).  For
 * the probability q = h_q[k]: h = (double)(n - 1) * q, j = floor(h), g = h - j, and
 *   d_bands[b][k][s] = (float) x_(j)                                                        when g == 0,
 *                      (float)((double)x_(j) + g * ((double)x_(j+1) - (double)x_(j)))        otherwise,
 * every FP64 operation rounded on its own: the "linear" (type 7) quantile, what numpy computes from a sort in the same IEEE operations.
 * n = 0 gives zero bands, n = 1 that replica's row for every q.  B == 0, M == 0 or Q == 0 returns 0 and does nothing.  A NULL plan,
 * d_rows, h_q or d_bands, ld < max, Q > 8 and a q that is NaN or outside [0, 1] return TSPWS_E_ARG ("replica_bands: ...") before any device
 * work, outputs untouched; the checks that need no plan come first.
 * One workgroup owns (ensemble, tile of 64 samples): M <= lds_max_rows stages the participating rows of its tile in LDS as keys (read
 * from HBM once) and selects per lane, bit by bit; a larger M runs the same selection on columns read from global memory.  The route
 * depends on M alone.  In rounds of whole ensembles (at most 65535 a round; the rows a round reads and its tables within TSPWS_PART_MB,
 * one ensemble alone may exceed it); per round one small table (the participating rows of every ensemble, j and g of every (ensemble, q))
 * is uploaded into a scratch slot of the unit's own.  Columns max .. ld-1 of d_rows are never read, nothing outside [B][Q][max] of d_bands
 * is written, nothing is atomic: a repeated call is bit-identical.  The call waits for `stream`: on return the bands are complete. */
int  tspws_hip_replica_bands(tspws_hip_plan *plan, const float *d_rows, size_t ld, unsigned B, unsigned M, const unsigned *h_mtr,
                             const double *h_q, unsigned Q, float *d_bands, void *stream);
/* How the plan's last tspws_hip_replica_bands call with B, M, Q > 0 went (zero before the first one; lds_max_rows is always set). */
typedef struct {
	unsigned lds;          /* ensembles selected from keys staged in LDS (M <= lds_max_rows)  */
	unsigned global;       /* ensembles selected from columns in global memory (M above that) */
	unsigned empty;        /* ensembles without a participating replica (zero bands)          */
	unsigned rounds;       /* rounds of whole ensembles                                       */
	unsigned lds_max_rows; /* the largest M that takes the LDS route                          */
} tspws_hip_bands_stats;
int  tspws_hip_replica_bands_stats(const tspws_hip_plan *plan, tspws_hip_bands_stats *stats);

/* ---- trace scores and the selective stack ---- */
/* Which traces belong in the stack: the reference's two figures of merit (similarity, ts_pws1f_lib.c:433-449; misfit, :452-462) of every
 * TRACE of B ensembles against R reference rows per ensemble, in one pass that reads every trace sample of the lag window once.  Ensemble
 * b = the traces [h_first[b], h_first[b+1]) of d_sigall (the rules of tspws_hip_stack_batch: B + 1 non-decreasing host offsets, h_first[0]
 * may be > 0, ld >= max), T = h_first[B] - h_first[0].  d_ref is [B][R][ldr] floats on the plan's device, 1 <= R <= 4, ldr >= max: row
 * (b, k) is reference k of ensemble b (R = 2 with the ls and tsPWS rows of tspws_hip_stack_batch scores against both at once).  The lag
 * window is the samples n0 <= n < n1, n0 < n1 <= max; n1 == 0 means max.  d_scores is [R][3][T] doubles on the device, the planes sim,
 * misfit, dot, column i - h_first[0] for trace i; d_energy is NULL or [T] doubles.  For trace x of ensemble b and r = row (b, k), every sum
 * over the window in FP64:
 *   dot = sum (double)x[n] (double)r[n], xx = sum (double)x[n]^2, rr = sum (double)r[n]^2, misfit = sum ((double)x[n] - (double)r[n])^2,
 *   sim = dot / sqrt(xx) / sqrt(rr) (the reference's similarity with the trace as x1), d_energy[i] = xx.
 * A trace or a reference without energy gives the reference's NaN for sim (0 / 0) -- NaN fails every >=, so a dead trace is never
 * selected; misfit, dot and the energy stay finite.  The order of every sum is fixed (nothing is atomic): a repeated call is bit-identical,
 * and the scores of a trace depend only on that trace, its reference rows, the window and the load route -- a batch and a loop of
 * one-ensemble calls on the same route give bit-equal columns, plane k of an R-reference call is that of the R = 1 call on reference k.
 * The route: 16-byte non-temporal loads iff max % 4 == 0, ld % 4 == 0, ldr % 4 == 0 and both bases are 16-byte aligned, scalar loads
 * otherwise; a window edge that is no multiple of 4 is a scalar head / tail.  Columns max .. ld-1 / ldr-1 are never read, nothing outside
 * the two outputs is written.  Two levels: one wave per (up to 4 consecutive traces of an ensemble, column segment of 4096 samples) leaves
 * partial sums in a scratch block that stays within TSPWS_PART_MB (rounds of whole ensembles; one ensemble alone may exceed it), a small
 * kernel adds the segments in segment order.  B == 0 or T == 0 returns 0 and does nothing; an empty ensemble has no columns.  NULL plan /
 * h_first / d_ref / d_scores, NULL traces with T > 0, decreasing offsets, ld < max, ldr < max, R == 0, R > 4, n0 >= n1 (after the n1 == 0
 * rule) and n1 > max return TSPWS_E_ARG ("trace_scores: ...") before any device work, outputs untouched; the checks that need no plan come
 * first.  So does a round that would need more than 2^33 waves (groups of 4 traces x column segments: one ensemble of 2^26 traces of
 * 2^21 samples).  The call uploads one small table per round and waits for `stream`: on return the outputs are complete. */
int  tspws_hip_trace_scores(tspws_hip_plan *plan, const float *d_sigall, size_t ld, const size_t *h_first, unsigned B, const float *d_ref,
                            size_t ldr, unsigned R, size_t n0, size_t n1, double *d_scores, double *d_energy, void *stream);
/* How the plan's last tspws_hip_trace_scores call with T > 0 went (all zero before the first one).  The figures are set when the call has
 * passed its refusals, before its device work: a call that then fails in the runtime leaves the figures of its plan.  The calls that
 * tspws_hip_selective_stack_batch makes count: after it the figures are those of its last scoring pass. */
typedef struct {
	unsigned vec;      /* 1: the 16-byte vector route, 0: the scalar route                 */
	unsigned segments; /* column segments per trace                                        */
	unsigned rounds;   /* rounds of whole ensembles                                        */
	unsigned empty;    /* ensembles without traces                                         */
} tspws_hip_trace_scores_stats_t;
int  tspws_hip_trace_scores_stats(const tspws_hip_plan *plan, tspws_hip_trace_scores_stats_t *stats);
/* Host: one mask row from one plane of scores.  score is [T] doubles (usually sim of one reference), T = first[B] - first[0]; sel receives
 * [T] bytes (1 = kept: one row of h_sel with M = 1), kept is NULL or receives the [B] kept counts.
 *   rule 0: keep iff score >= a.
 *   rule 1: per ensemble over its FINITE scores, med = the median (an even count: 0.5 * (lo + hi) of the two middle order statistics),
 *           mad = the median of fabs(score - med) by the same rule; keep iff score >= med - a * 1.4826 * mad, evaluated left to right in FP64.
 * NaN is never kept; an ensemble without a finite score keeps nothing.  Returns 0; 1 for NULL sel / score / first or decreasing offsets
 * (nothing written); 2 for an unknown rule or a NaN a (nothing written). */
int  tspws_selection_from_scores(char *sel, unsigned *kept, const double *score, const size_t *first, unsigned B, int rule, double a);
/* The selective stack of B ensembles: stack, score, select, restack, built from tspws_hip_stack_batch, tspws_hip_trace_scores (R = 1),
 * tspws_selection_from_scores (on the sim plane) and tspws_hip_subsample_batch_sel (M = 1); no kernel of its own.  against: 0 scores
 * against the ls row, 1 against the tsPWS row; rule / a as in tspws_selection_from_scores; n0 / n1 the lag window of the scores; iters >= 1.
 * Pass 0: the plain stacks give the rows, every trace is scored against the chosen one, the mask is selected and the ensembles are
 * restacked with it into d_ls / d_tsPWS ([B][max]) and h_kept ([B]).  Every further pass scores ALL traces against the rows the previous
 * pass wrote and selects again: an unchanged mask ends the call, otherwise the ensembles are restacked.  *iters_done (NULL: not wanted) =
 * the number of restacks, h_sel[T] = the last mask used: the final rows are, bit for bit, what tspws_hip_subsample_batch_sel(M = 1, h_sel)
 * writes, with its definitions -- ls is that call's time-domain row (not the frame-filtered ls of tspws_hip_stack), an ensemble is
 * two-stage by M_b (not by the kept count), an ensemble that keeps nothing gives zero rows and count 0.  NULL plan / p / h_first / outputs
 * / h_sel / h_kept, NULL traces with T > 0, decreasing offsets, ld < max, against outside {0, 1}, an unknown rule, a NaN a, iters == 0
 * and a bad window return TSPWS_E_ARG ("selective_stack_batch: ...") before any device work, outputs untouched; the checks that need no
 * plan come first; an ensemble of more than 2^32 - 16 traces is refused there too (the limit of tspws_hip_subsample_batch_sel, checked
 * up front so that no stack is computed first).  What only a composed call can judge -- a parameter set that tspws_hip_stack_batch
 * rejects, a failed allocation, a runtime error -- returns that call's code with that call's error text ("stack_batch: ...",
 * "subsample_batch: ...", "trace_scores: ..."), possibly after earlier passes have written the outputs.  The call overwrites the plan's
 * stack_batch, trace_scores and subsample_batch statistics.  B == 0 returns 0 and does nothing.  Fold and mean removal stay with the
 * caller.  Every composed call waits for `stream`: on return the outputs are complete. */
int  tspws_hip_selective_stack_batch(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, const size_t *h_first, unsigned B,
                                     int against, int rule, double a, unsigned iters, size_t n0, size_t n1, float *d_ls, float *d_tsPWS,
                                     char *h_sel, unsigned *h_kept, unsigned *iters_done, void *stream);

/* ---- dv/v by stretching of stack rows ---- */
/* The stretching estimate of dv/v for the rows the batched calls leave: per (row, window) the correlation coefficient of the row with its
 * ensemble's reference row evaluated at lag t (1 + eps), on a grid of E stretch factors, and the maximum with a three-point fit.
 * d_rows is [B][M][ld] floats on the plan's device (d_ls_out / d_ts_out of the batched calls: ld >= max = N), h_mtr NULL or [B][M] host
 * counts: row (b, m) takes part iff h_mtr == NULL or h_mtr[b][m] > 0 (tspws_hip_replica_bands' rule).  d_ref is [B][ldr] floats, one
 * reference row per ensemble, ldr >= max (band rows [B][R][max]: B R ensembles of M = 1).  z is the zero-lag position in samples; it may be
 * fractional or outside [0, N).  h_eps[E] increases strictly, |eps| <= 0.5, 1 <= E <= 4096.  h_win holds W pairs [n0_w, n1_w),
 * n0 < n1 <= N, 1 <= W <= 4; windows may overlap.
 * Definition, in FP64 with every operation rounded on its own (no contraction): for sample n and stretch e
 *   u = (double)n + ((double)n - z) * eps_e, i = floor(u), f = u - i,
 *   w-1 = ((-0.5 f + 1) f - 0.5) f,  w0 = (1.5 f - 2.5) f f + 1,  w1 = ((-1.5 f + 2) f + 0.5) f,  w2 = (0.5 f - 0.5) f f
 *   S_e[n] = ((w-1 ref[i-1] + w0 ref[i]) + w1 ref[i+1]) + w2 ref[i+2]     (cubic convolution, Keys a = -1/2; samples outside [0, N) are zero)
 * so eps = 0 gives S[n] = ref[n] exactly; and per (b, m, w, e), over n0_w <= n < n1_w with c the row,
 *   dot = sum (double)c[n] S_e[n],   cc = dot / sqrt(sum c^2) / sqrt(sum S_e^2)      (the reference's similarity order)
 * A dead row or a dead stretched reference gives the reference's NaN (0 / 0).  With this definition cur(t) = ref(t (1 + eps)), so the eps
 * of the maximum is dv/v.
 * d_cc is NULL or [B][M][W][E] doubles; d_fit is [B][M][W][4] doubles: eps_hat, cc_hat, (double)e*, edge.  e* = the first index of the largest
 * non-NaN cc.  With c- = cc[e* - 1], c0 = cc[e*], c+ = cc[e* + 1]: when 0 < e* < E - 1 and den = c- - 2 c0 + c+ != 0,
 *   d = 0.5 (c- - c+) / den,  eps_hat = eps[e*] + d * (d >= 0 ? eps[e* + 1] - eps[e*] : eps[e*] - eps[e* - 1]),
 *   cc_hat = c0 - 0.25 (c- - c+) d,  edge = 0;
 * otherwise eps_hat = eps[e*], cc_hat = c0, edge = 1.  Without a non-NaN cc, or for a row that does not take part, d_fit is NaN, NaN, -1, 1
 * and the row's d_cc entries are NaN.
 * Nothing is atomic and every sum has a fixed order: a repeated call is bit-identical, and the values of (b, m, w, e) depend only on that
 * row, its reference, z, eps_e and window w -- not on B, M, the other grid entries, the other windows, the rounds or a tile's padding.
 * Three kernels: the stretched references S of a round in FP64 (built once per ensemble, shared by its M rows) with the per-segment sums
 * of S^2; the contraction rows . S on v_mfma_f64_16x16x4_f64, one wave per (up to 32 rows, up to 64 stretches, segment of 512 window
 * samples), which also leaves sum c^2; a final kernel that adds the segments in segment order, forms cc and the fit.  In rounds of (whole
 * ensembles x chunks of the grid in multiples of 16) so that S and the partial sums stay within TSPWS_PART_MB (one ensemble x 16 stretches
 * alone may exceed it); one small table upload per round into scratch slots of the unit's own.
 * NULL plan / d_rows / d_ref / h_eps / h_win / d_fit, ld < max, ldr < max, E or W outside its range, a grid that does not increase strictly,
 * a NaN grid entry or one with |eps| > 0.5, a NaN or infinite z, and a bad window (n0 >= n1, n1 > max) return TSPWS_E_ARG
 * ("stretch_rows: ...") before any device work, outputs untouched; the checks that need no plan come first.  So do more than 2^32 - 16 rows.
 * B == 0 or M == 0 returns 0 and does nothing.  Columns max .. ld-1 / ldr-1 are never read, nothing outside the two outputs is written.
 * The call waits for `stream`: on return the outputs are complete. */
int  tspws_hip_stretch_rows(tspws_hip_plan *plan, const float *d_rows, size_t ld, unsigned B, unsigned M, const unsigned *h_mtr,
                            const float *d_ref, size_t ldr, double z, const double *h_eps, unsigned E, const size_t *h_win, unsigned W,
                            double *d_cc, double *d_fit, void *stream);
/* How the plan's last tspws_hip_stretch_rows call with B, M > 0 went (all zero before the first one). */
typedef struct {
	unsigned rounds;   /* rounds of whole ensembles                                  */
	unsigned segments; /* column segments of the window set (all windows together)   */
	unsigned rows;     /* rows that took part                                        */
	unsigned left_out; /* rows left out by h_mtr                                     */
	unsigned chunks;   /* chunks of the stretch grid per round (the largest count)   */
} tspws_hip_stretch_stats;
int  tspws_hip_stretch_rows_stats(const tspws_hip_plan *plan, tspws_hip_stretch_stats *stats);
/* Host: the symmetric stretch grid eps[e] = ((double)e - h) * (eps_max / h), h = (E - 1) / 2, for an odd E >= 3: the middle entry is
 * exactly 0.  Returns 0; 1 for NULL eps; 2 for an even E, E < 3 or an eps_max outside (0, 0.5] (nothing written). */
int  tspws_stretch_grid(double *eps, double eps_max, unsigned E);

/* ---- dv/v per band from the wavelet cross-spectrum ---- */
/* The time-frequency estimate of dv/v: the phase of the wavelet cross-spectrum between a row and its ensemble's reference becomes a delay
 * per coefficient, and per (row, window, band of scales) the delay is regressed on the lag.  The frequency-resolved companion of
 * tspws_hip_stretch_rows: rows, counts, references, z and windows mean what they mean there (row (b, m) takes part iff h_mtr == NULL or
 * h_mtr[b][m] > 0; z, the zero-lag position in samples, may be fractional; 1 <= W <= 4 windows [n0, n1), n0 < n1 <= N, which may overlap).
 * h_bands holds 1 <= R <= 64 half-open scale ranges as for tspws_hip_inverse_bands: they may overlap, cut an octave between voices, be empty.
 * Definition.  Coefficient k < N_s of scale s sits at sample k D_s.  With c = Yc_s[k] of the row's set and r = Yr_s[k] of the reference's, in FP64:
 *   xr = c.re r.re + c.im r.im,  xi = c.im r.re - c.re r.im   (X = c conj(r)),   a = hypot(xr, xi),   phi = atan2(xi, xr)
 *   omega_s = w0 / scale_s   (rad per sample: 2 PI dt times the centre frequency of tspws_bands_from_frequencies)
 *   delta = phi / omega_s,   t = (double)(k D_s) - z
 * The coefficient takes part in (w, band) iff s lies in the band, n0_w <= k D_s < n1_w, a is finite and > 0, and -- with skip_wrapped != 0 --
 * its filter support [k D_s - c_s, k D_s - c_s + L_s) lies inside [0, N) (c_s, L_s: tspws_hip_plan_tables), which leaves out the coefficients that
 * mix the two trace ends through the circular correlation.  d_sums is NULL or [..][W][R][9] doubles, over the coefficients that take part:
 *   n (as a double), A = sum a, At = sum a t, Att = sum a t^2, Ad = sum a delta, Atd = sum a t delta, Add = sum a delta^2, Xr = sum xr, Xi = sum xi
 * d_fit is [..][W][R][6] doubles from those sums, every operation rounded on its own (no contraction):
 *   den = A Att - At At
 *   eps_hat = (A Atd - At Ad) / den        (the slope of the delay on the lag: dv/v)
 *   icpt    = (Att Ad - At Atd) / den      (samples)
 *   res     = (Add - icpt Ad) - eps_hat Atd,   rms = sqrt((res > 0 ? res : 0) / A)
 *   err     = rms sqrt(A / den)            (the slope's standard error per effective observation)
 *   coh     = hypot(Xr, Xi) / A            (the hypot with one correction step: the correctly rounded value in all but rare cases)
 *   fit = eps_hat, icpt, err, rms, coh, n
 * n < 2 or !(den > 0) gives NaN, NaN, NaN, NaN, coh, n, with coh NaN when A == 0.  A row that does not take part gives five NaN and n = -1, and
 * NaN sums.  With the library's Y, a row cur(t) = ref(t (1 + eps)) has delta ~ eps t: eps_hat is dv/v in the sign of tspws_hip_stretch_rows.
 * The phase is NOT unwrapped: the estimate needs |omega_s eps t| < PI inside the window; that is the caller's choice of bands and windows.
 * Nothing is atomic and every sum has a fixed order: a repeated call is bit-identical, and the sums of (row, w, band) depend only on that
 * row's and its reference's coefficients, z, the window, the band and skip_wrapped -- not on nrow, B, M, the other bands and windows, the
 * rounds or any padding.  The unit of work is (row, scale inside at least one band, window, segment of 256 coefficients of the window's index
 * range of that scale, counted from its first index); a wave takes a run of short items one after the other; a final kernel adds a band's
 * scales in increasing s and each scale's segments in increasing order (the principle of tspws_hip_inverse_bands' combining kernel).
 *
 * tspws_hip_wxs_coef: on coefficient sets.  d_Yc is [nrow][ncoef] complex, d_Yr [B][ncoef] complex (tspws_hip_forward_f32's layout); h_ens[nrow]
 * names the reference set of every row (NULL: nrow == B, row i against set i); outputs [nrow][W][R][9] / [6].  In chunks of rows whose
 * partial sums stay within TSPWS_PART_MB.
 * tspws_hip_wxs_rows: on rows.  d_rows is [B][M][ld] floats, d_ref [B][ldr] floats; outputs [B][M][W][R][9] / [6].  In rounds of whole ensembles
 * whose coefficient sets ((M + 1) ncoef complex each) and partial sums stay within TSPWS_PART_MB (one ensemble alone may exceed it); a round
 * is ONE tspws_hip_forward_f32 call on its rows (those left out are transformed too), one on its references, and one pass of the two kernels.
 * NULL plan / inputs / h_bands / h_win / d_fit, ld < max, ldr < max, R or W outside its range, s_begin > s_end, s_end > S, a bad window (n0 >= n1,
 * n1 > max), a NaN or infinite z, an h_ens entry >= B (or no h_ens with nrow != B) and more than 2^32 - 16 rows return TSPWS_E_ARG
 * ("wxs_coef: ..." / "wxs_rows: ...") before any device work, outputs untouched; the checks that need no plan come first.  B == 0, M == 0 or
 * nrow == 0 returns 0 and does nothing.  Columns max .. ld-1 / ldr-1 are never read, nothing outside the two outputs is written; one small table
 * upload per pass into scratch slots of the unit's own.  The calls wait for `stream`: on return the outputs are complete. */
int  tspws_hip_wxs_coef(tspws_hip_plan *plan, const double *d_Yc, const double *d_Yr, const unsigned *h_ens, size_t nrow, unsigned B, double z,
                        const tspws_band *h_bands, unsigned R, const size_t *h_win, unsigned W, int skip_wrapped, double *d_sums, double *d_fit,
                        void *stream);
int  tspws_hip_wxs_rows(tspws_hip_plan *plan, const float *d_rows, size_t ld, unsigned B, unsigned M, const unsigned *h_mtr, const float *d_ref,
                        size_t ldr, double z, const tspws_band *h_bands, unsigned R, const size_t *h_win, unsigned W, int skip_wrapped,
                        double *d_sums, double *d_fit, void *stream);
/* How the plan's last tspws_hip_wxs_rows / tspws_hip_wxs_coef call that did work went (all zero before the first one). */
typedef struct {
	unsigned rounds;   /* rounds of whole ensembles (wxs_coef: chunks of rows)       */
	unsigned rows;     /* rows that took part                                        */
	unsigned left_out; /* rows left out by h_mtr                                     */
	unsigned items;    /* work items per row: (scale, window, segment)               */
	unsigned scales;   /* scales inside at least one band                            */
} tspws_hip_wxs_stats;
int  tspws_hip_wxs_rows_stats(const tspws_hip_plan *plan, tspws_hip_wxs_stats *stats);

/* ---- dv/v by the moving-window cross-spectrum (MWCS; Clarke et al. 2011) -------------------------------------------------
 * Rows, counts, references, z and the lag ranges as for tspws_hip_stretch_rows: d_rows is [B][M][ld] floats, h_mtr NULL or [B][M] (row (b, m)
 * takes part iff h_mtr == NULL or the count is > 0), d_ref [B][ldr] floats, z may be fractional or outside [0, max), h_win holds 1 <= W <= 4
 * pairs [n0_w, n1_w), n0 < n1 <= max, which may overlap.
 * Parameters: L = window length in samples, 16 <= L <= 1024 (any L, no multiple of 4 needed); 1 <= hop <= L; P = DFT length, a power of two,
 * L <= P <= 4096; [q0, q1) = the band as DFT bins, 1 <= q0, q0 + 2 <= q1 <= P/2 (tspws_mwcs_bins makes them from frequencies); h = smoothing
 * half-width in bins, 0 <= h <= 8; taper = the fraction of the window under the cosine taper, in [0, 1]; min_coh, max_err, max_delta = the
 * filters of stage 3 (max_err, max_delta may be +inf); err_floor > 0.  The extended bin range is [qa, qb) = [max(0, q0 - h),
 * min(P/2 + 1, q1 + h)), Qx = qb - qa <= 64.
 * WINDOWS.  Range w holds J_w = (n1_w - n0_w >= L) ? (n1_w - n0_w - L) / hop + 1 : 0 windows starting at n_j = n0_w + j hop; J = sum J_w,
 * 1 <= J <= 4096; the windows are numbered range after range; t_j = ((double)n_j + 0.5 (L - 1)) - z.
 * STAGE 1, spectra.  tspws_mwcs_basis writes the table the device uses (tspws_mwcs_basis_size doubles: g[L] | C[L][Qx] | S[L][Qx] | Tc[Qx] |
 * Ts[Qx] | k[2 h + 1] | v[Qx]): g = the cosine taper -- with a = taper L / 2 and x = min(l + 1/2, L - 1/2 - l), g[l] = 0.5 (1 - cos(PI x / a))
 * for x < a, else 1 --, C[l][q] = g[l] cos(2 PI ((q l) mod P) / P), S[l][q] = -g[l] sin(same) for q in [qa, qb), every entry rounded to
 * double once; Tc[q] = sum_l C[l][q], Ts likewise, added in ascending l; k[d + h] = 0.5 (1 + cos(PI d / (h + 1))); v[q] = 2 PI q / P.  The
 * device never evaluates a sine.  For a window x[l] = (double)row[n_j + l], in FP64: mu = (sum_l x[l]) / L and
 * F[q] = (sum_l x[l] C[l][q] - mu Tc[q]) + i (sum_l x[l] S[l][q] - mu Ts[q]), the demeaned, tapered window's DFT bin q of length P; the sums
 * over l in any order (the matrix pipe).  The reference's windows go through the same code as one more row of their ensemble.
 * STAGE 2, per (row, window); from here every FP64 operation is rounded on its own, in the stated order.  With c = F of the row, r = F of
 * the reference, per bin of [qa, qb): Xr = c.re r.re + c.im r.im, Xi = c.im r.re - c.re r.im, Pc = c.re c.re + c.im c.im, Pr likewise.
 * For q in [q0, q1) and each of the four planes sm(v)[q] = (sum_{d = -h..h, qa <= q + d < qb} k[d] v[q + d]) / (sum of the same k[d]),
 * both sums from 0 in ascending d.  a = hypot(smXr, smXi), coh = a / sqrt(smPc smPr), phi = atan2(smXi, smXr) (not unwrapped:
 * |v delta| < PI is the caller's choice of band and ranges), cc = min(coh, 0.99), wq = sqrt(cc cc / (1 - cc cc) * sqrt(a)).  In ascending
 * q: Svv = sum (wq v) v, Svp = sum (wq v) phi; delta = Svp / Svv, in samples; s2 = (sum (phi - delta v)^2) / (nq - 1), nq = q1 - q0;
 * err = sqrt((sum (wq v)(wq v)) s2) / Svv; mcoh = (sum coh) / nq.  A row cur(t) = ref(t (1 + eps)) has delta ~ eps t.  A bin with
 * smPc smPr == 0 gives the window delta = err = mcoh = NaN.  d_win is NULL or [B][M][J][3] = delta, err, mcoh.
 * STAGE 3, per (row, range).  Window j takes part iff delta and err are finite, err <= max_err, mcoh >= min_coh and |delta| <= max_delta.
 * p = 1 / (e e), e = max(err, err_floor); in ascending j: S = sum p, St = sum (p t), Stt = sum (p t) t, Sd = sum p delta,
 * Std = sum (p t) delta; den = S Stt - St St; eps_hat = (S Std - St Sd) / den, icpt = (Stt Sd - St Std) / den, err_eps = sqrt(S / den);
 * eps0 = Std / Stt and err0 = sqrt(1 / Stt), the fit through the origin.  d_fit is [B][M][W][6] = eps_hat, icpt, err_eps, eps0, err0, n.
 * n < 2 or !(den > 0) gives NaN for the first three; the through-origin pair stands when n >= 1 and Stt > 0 (else NaN).  A row that does not
 * take part gives five NaN and n = -1, and NaN in d_win and d_spec.  eps_hat is dv/v in the sign of stretch_rows and wxs_rows.
 * d_spec (NULL or [B][M][J][Qx] complex) and d_spec_ref (NULL or [B][J][Qx] complex) return stage 1.
 * Nothing is atomic, every output has one writer: a repeated call is bit-identical, and the values of (b, m, j) depend on that row, its
 * reference, the window and the parameters alone -- not on B, M, the other ranges, the rounds (whole ensembles whose spectra and window
 * results stay within TSPWS_PART_MB; one ensemble alone may exceed it) or a tile's padding.
 * NULL plan / rows / ref / par / h_win / d_fit, ld < max, ldr < max, a parameter outside its range, Qx > 64, J > 4096, J == 0, a bad range
 * (n0 >= n1, n1 > max), a NaN or infinite z and more than 2^32 - 16 rows return TSPWS_E_ARG ("mwcs_rows: ...") before any device work, outputs
 * untouched; the checks that need no plan come first.  B == 0 or M == 0 returns 0 and does nothing.  Columns max .. ld-1 / ldr-1 are never
 * read, nothing outside the outputs is written; one table upload per round into scratch slots of the unit's own.  The call waits for
 * `stream`: on return the outputs are complete. */
typedef struct {
	unsigned L, hop, P, q0, q1, h;
	double taper, min_coh, max_err, max_delta, err_floor;
} tspws_mwcs_par;
/* The bins with f_lo <= q / (P dt) < f_hi, without bin 0 and below P/2: q0 = max(1, ceil(f_lo P dt)), q1 = min(P/2, ceil(f_hi P dt)).
 * Returns 0; 1: NULL; 2: P no power of two in [16, 4096], dt <= 0, f_lo < 0 or f_hi <= f_lo; 3: fewer than two bins. */
int    tspws_mwcs_bins(unsigned P, double dt, double f_lo, double f_hi, unsigned *q0, unsigned *q1);
size_t tspws_mwcs_basis_size(const tspws_mwcs_par *par);          /* doubles of the table; 0 for parameters the call would refuse */
int    tspws_mwcs_basis(const tspws_mwcs_par *par, double *tab);  /* 0; 1: NULL; 2: parameters the call would refuse */
int  tspws_hip_mwcs_rows(tspws_hip_plan *plan, const float *d_rows, size_t ld, unsigned B, unsigned M, const unsigned *h_mtr, const float *d_ref,
                         size_t ldr, double z, const tspws_mwcs_par *par, const size_t *h_win, unsigned W, double *d_win, double *d_fit,
                         double *d_spec, double *d_spec_ref, void *stream);
/* How the plan's last tspws_hip_mwcs_rows call with B, M > 0 went (all zero before the first one). */
typedef struct {
	unsigned rounds;   /* rounds of whole ensembles                                  */
	unsigned rows;     /* rows that took part                                        */
	unsigned left_out; /* rows left out by h_mtr                                     */
	unsigned windows;  /* J: windows of all lag ranges                               */
	unsigned bins;     /* Qx: bins of the band with the smoothing margins            */
} tspws_hip_mwcs_stats;
int  tspws_hip_mwcs_rows_stats(const tspws_hip_plan *plan, tspws_hip_mwcs_stats *stats);

/* ---- dv/v by dynamic time warping (DTW; Hale 2013, Mikesell et al. 2015) --------------------------------------------------
 * The delay as a function of lag: per (row, lag range) the integer lag path that aligns the row with its ensemble's reference at the smallest
 * accumulated squared error, and the regression of that path on the lag.  Unlike the cross-spectral estimates it survives a cycle skip, and
 * it returns delta(t) itself.  Rows, counts, references, z and the lag ranges as for tspws_hip_stretch_rows: d_rows is [B][M][ld] floats, h_mtr
 * NULL or [B][M] (row (b, m) takes part iff h_mtr == NULL or the count is > 0), d_ref [B][ldr] floats, z may be fractional or outside
 * [0, max), h_win holds 1 <= W <= 4 pairs [n0_w, n1_w), n0 < n1 <= max, which may overlap.
 * Parameters: 1 <= Lmax <= 127, the largest lag: nl = 2 Lmax + 1 lags l = -Lmax .. Lmax; 1 <= b <= 8, the strain limit: the lag changes by at
 * most one sample per b samples.  n_w = n1_w - n0_w <= 131072 for every range (the integer sums below are then exact in a double);
 * T = sum_w n_w.
 * DEFINITION.  Every FP64 operation is rounded on its own, in the stated order, with no contraction anywhere.  For row c, reference r,
 * range w, N = max, i = 0 .. n_w - 1, n = n0_w + i:
 * 1. Normalisation.  mc = max_i |c[n]|; mr = max |r[k]| over k in [max(0, n0_w - Lmax), min(N, n1_w + Lmax)); both in float, hence exact.
 *    ac = 1.0 / (double)mc, ar = 1.0 / (double)mr.  mc == 0, mr == 0, a non-finite mc or mr, or a NaN among those samples makes the
 *    (row, range) DEAD.
 * 2. Error.  e[i][l] = d d, d = (double)c[n] ac - (double)r[clamp(n + l, 0, N - 1)] ar: both products rounded before the subtraction; a lag
 *    that points outside the trace takes the nearest sample inside.
 * 3. Accumulation, ascending i.  D[0][l] = e[0][l].  For i >= 1, ib = max(0, i - b): dc = D[i-1][l]; for l > -Lmax, dm = D[ib][l-1], then
 *    dm = dm + e[k][l-1] for k = i-1 down to ib+1, else dm = +inf; dp likewise with l+1 (+inf at l = Lmax).  The choice is C if dc <= dm &&
 *    dc <= dp, else Mn if dm <= dp, else Pl; D[i][l] = e[i][l] + (the chosen one of dc, dm, dp).
 * 4. Backtracking.  l* = the first l in ascending order with the smallest D[n_w-1][l]; lag[n_w-1] = l*.  At (i, l): choice C gives
 *    lag[i-1] = l, continue at (i-1, l); Mn gives lag[k] = l-1 for k = i-1 .. ib, continue at (ib, l-1); Pl the same with l+1.  Stop at i = 0.
 * 5. Fit.  As 64-bit integers, then converted to double (all exact): S = n_w, Si = sum i, Sii = sum i^2, Sl = sum lag[i], Sil = sum i lag[i],
 *    Sll = sum lag[i]^2, clip = the number of i with |lag[i]| == Lmax.  Then
 *      den = S Sii - Si Si,   num = S Sil - Si Sl,   eps_hat = num / den,   t0 = ((double)n0_w - z) + Si / S,   icpt = Sl / S - eps_hat t0
 *      res = (Sll - (Sl / S) Sl) - eps_hat (num / S),   rms = sqrt((res > 0 ? res : 0) / S),   err = rms sqrt(S / den)
 *      dist = D[n_w-1][l*] / S
 * d_fit is [B][M][W][6] doubles = eps_hat, icpt, err, rms, dist, clip (n_w is the caller's own n1_w - n0_w and is not returned).  icpt is the lag
 * at z, in samples; eps_hat the slope of the lag on n - z: a row cur(t) = ref(t (1 + eps)) has its best match at lag ~ eps t, so eps_hat is dv/v
 * in the sign of stretch_rows, wxs_rows and mwcs_rows.  n_w == 1 (den == 0) gives NaN for eps_hat, icpt and err; rms (0), dist and clip stand.
 * A dead (row, range) and a row that does not take part give five NaN and clip = -1, and lags INT_MIN.
 * d_lag is NULL or [B][M][T] ints: the path of range w at [off_w, off_w + n_w), off_w = sum of the n of the ranges before it.
 * Nothing is atomic, every output has one writer: a repeated call is bit-identical, and the values of (b, m, w) depend on that row, its
 * reference, z, the range and par alone -- not on B, M, the other ranges, the rounds or any padding.  One wave takes a (row, range): the
 * lags on the lanes (1, 2 or 4 consecutive lags each), two bits of choice per (sample, lag) in the wave's plane of ceil(n_w / 16) x 64 ceil(nl / 64)
 * 32-bit words in plan scratch, the same wave backtracks.  The call runs in rounds of whole ensembles whose planes stay within TSPWS_PART_MB
 * (one ensemble alone may exceed it), one table upload per round into scratch slots of the unit's own.
 * NULL plan / rows / ref / par / h_win / d_fit, ld < max, ldr < max, Lmax, b or W outside its range, a bad range (n0 >= n1, n1 > max, longer
 * than 131072), a NaN or infinite z and more than 2^32 - 16 rows return TSPWS_E_ARG ("dtw_rows: ...") before any device work, outputs
 * untouched; the checks that need no plan come first.  B == 0 or M == 0 returns 0 and does nothing.  Columns max .. ld-1 / ldr-1 are never
 * read, nothing outside the outputs is written.  The call waits for `stream`: on return the outputs are complete. */
typedef struct { unsigned Lmax, b; } tspws_dtw_par;
int  tspws_hip_dtw_rows(tspws_hip_plan *plan, const float *d_rows, size_t ld, unsigned B, unsigned M, const unsigned *h_mtr, const float *d_ref,
                        size_t ldr, double z, const tspws_dtw_par *par, const size_t *h_win, unsigned W, int *d_lag, double *d_fit, void *stream);
/* How the plan's last tspws_hip_dtw_rows call with B, M > 0 went (all zero before the first one). */
typedef struct {
	unsigned rounds;   /* rounds of whole ensembles                                  */
	unsigned rows;     /* rows that took part                                        */
	unsigned left_out; /* rows left out by h_mtr                                     */
	unsigned lags;     /* nl = 2 Lmax + 1                                            */
	unsigned samples;  /* T: samples of all lag ranges                               */
} tspws_hip_dtw_stats;
int  tspws_hip_dtw_rows_stats(const tspws_hip_plan *plan, tspws_hip_dtw_stats *stats);

/* ---- group arrivals per scale (frequency-time analysis) ---- */
/* The dispersion measurement on the rows the batched calls leave: the complex Morlet frame is a bank of narrow-band filters, and per (row,
 * window, scale) the peaks of the envelope inside a velocity window are the group arrivals of that period (tspws_ftan_periods), with the
 * coefficient at the peak (its phase and the phase velocity are the caller's: the device evaluates no atan2) and a noise level.  Rows, counts
 * and z as for tspws_hip_wxs_rows: [B][M][ld] floats, row (b, m) takes part iff h_mtr == NULL or h_mtr[b][m] > 0; z, the zero-lag position in
 * samples, may be fractional.  Scales [s_begin, s_end), s_begin < s_end <= S; Sx = s_end - s_begin.  h_win is [B][W][2]: 1 <= W <= 4 windows
 * [n0, n1), n0 < n1 <= N, PER ENSEMBLE (station pairs differ in distance; tspws_ftan_windows makes them), which may overlap.  h_noise is NULL
 * or [B][2]: a range [q0, q1), q0 < q1 <= N, per ensemble.  1 <= P <= 4 peaks are reported.
 * Definition.  Coefficient k < N_s of scale s sits at sample k D_s.  Every FP64 operation is rounded on its own (no contraction).  With
 * c = Y_s[k]:
 *   a2[k] = c.re c.re + c.im c.im
 * k is a member of window w iff n0 <= k D_s < n1 and -- with skip_wrapped != 0 -- its filter support [k D_s - c_s, k D_s - c_s + L_s) lies
 * inside [0, N) (the rule of tspws_hip_wxs_rows).  A member k is a peak iff 1 <= k <= N_s - 2, a2[k-1], a2[k] and a2[k+1] are all finite,
 * a2[k] > a2[k-1] and a2[k] >= a2[k+1].  The neighbours are indices of the scale, not members of the window: a peak at the window's first or
 * last member is a peak, the two ends of the scale never are, and on a plateau the left sample is the peak.  The peaks of (row, w, s) are
 * ordered by decreasing a2, ties by increasing k, and the first P are reported.  Per reported peak, with am = a2[k-1], a0 = a2[k],
 * ap = a2[k+1]:
 *   den = (am - 2.0 a0) + ap,   d = den != 0 ? 0.5 (am - ap) / den : 0   (the vertex of the parabola through the three, in indices)
 *   tg = ((double)k + d) (double)D_s - z   (the group arrival as a lag in samples),   amp = sqrt(a0)
 * d_peaks is [..][W][Sx][P][5] doubles: tg, amp, c.re, c.im, (double)k; c.re and c.im are exact copies.  The slots beyond the number of
 * peaks hold four NaN and k = -1, and so do the rows left out.  d_noise is NULL or [..][Sx][2] doubles and must be NULL when h_noise is
 * NULL: Q = the sum of the finite a2[k] whose k D_s lies in the ensemble's [q0, q1) (under the wrap rule when it is set) and their number as
 * a double; a row left out gives NaN and -1.  With d_noise == NULL h_noise is checked and not used.
 * Nothing is atomic and every output has one writer: a repeated call is bit-identical, and the values of (row, w, s) depend only on that
 * row's coefficients of scale s, the window, z and skip_wrapped -- not on B, M, nrow, the other windows, scales or ensembles, P, the rounds
 * or any padding; the P = 2 list is the head of the P = 4 list.  Ensembles whose windows (and noise ranges, when used) are equal by value
 * form a class; the unit of work is (row, scale, window or noise range, segment of 256 members counted from the range's first member) and a
 * wave takes a run of short items; a final kernel merges the segments' lists in segment order and adds the noise partials in that order.
 *
 * tspws_hip_ftan_coef: on coefficient sets.  d_Y is [nrow][ncoef] complex (tspws_hip_forward_f32's layout); h_ens[nrow] names the ensemble of
 * every row (NULL: nrow == B, row i of ensemble i); outputs [nrow][W][Sx][P][5] / [nrow][Sx][2].  In chunks of rows whose partial results
 * stay within TSPWS_PART_MB.
 * tspws_hip_ftan_rows: on rows.  Outputs [B][M][W][Sx][P][5] / [B][M][Sx][2].  In rounds of whole ensembles whose coefficient sets (M ncoef
 * complex each) and partial results stay within TSPWS_PART_MB (one ensemble alone may exceed it); a round is ONE tspws_hip_forward_f32 call
 * on its rows (those left out are transformed too) and one pass of the two kernels.
 * NULL plan / inputs / h_win / d_peaks, ld < max, W or P outside 1 .. 4, s_begin >= s_end, s_end > S, a bad window or noise range
 * (n0 >= n1, n1 > max), d_noise without h_noise, a NaN or infinite z, an h_ens entry >= B (or no h_ens with nrow != B) and more than
 * 2^32 - 16 rows return TSPWS_E_ARG ("ftan_coef: ..." / "ftan_rows: ...") before any device work, outputs untouched; the checks that need no
 * plan come first.  B == 0, M == 0 or nrow == 0 returns 0 and does nothing.  Columns max .. ld-1 are never read, nothing outside the two
 * outputs is written; one small table upload per pass into scratch slots of the unit's own.  The calls wait for `stream`: on return the
 * outputs are complete. */
int  tspws_hip_ftan_coef(tspws_hip_plan *plan, const double *d_Y, const unsigned *h_ens, size_t nrow, unsigned B, double z, unsigned s_begin,
                         unsigned s_end, const size_t *h_win, unsigned W, const size_t *h_noise, unsigned P, int skip_wrapped, double *d_peaks,
                         double *d_noise, void *stream);
int  tspws_hip_ftan_rows(tspws_hip_plan *plan, const float *d_rows, size_t ld, unsigned B, unsigned M, const unsigned *h_mtr, double z,
                         unsigned s_begin, unsigned s_end, const size_t *h_win, unsigned W, const size_t *h_noise, unsigned P, int skip_wrapped,
                         double *d_peaks, double *d_noise, void *stream);
/* How the plan's last tspws_hip_ftan_rows / tspws_hip_ftan_coef call that did work went (all zero before the first one). */
typedef struct {
	unsigned rounds;   /* rounds of whole ensembles (ftan_coef: chunks of rows)                      */
	unsigned rows;     /* rows that took part                                                        */
	unsigned left_out; /* rows left out by h_mtr                                                     */
	unsigned items;    /* work items of all classes: (scale, window or noise range, segment)         */
	unsigned classes;  /* classes of ensembles with equal windows (and noise ranges, when used)      */
} tspws_hip_ftan_stats;
int  tspws_hip_ftan_rows_stats(const tspws_hip_plan *plan, tspws_hip_ftan_stats *stats);
/* Host rule, no device: the windows of one station pair.  A surface wave of group velocity vmin .. vmax over the distance dist arrives at the
 * lags dist / (vmax dt) .. dist / (vmin dt) samples: win[0] = [ceil(z + dist / (vmax dt)), floor(z + dist / (vmin dt)) + 1) clipped to [0, N];
 * sides == 2 adds the mirrored acausal window win[1] = [ceil(z - dist / (vmin dt)), floor(z - dist / (vmax dt)) + 1).  win holds 2 sides
 * entries.  A NULL win, sides other than 1 or 2, a non-finite argument, dist < 0, vmin <= 0, vmax < vmin, dt <= 0 and an empty window after
 * clipping return TSPWS_E_ARG ("ftan_windows: ..."), nothing written. */
int  tspws_ftan_windows(double dist, double vmin, double vmax, double dt, double z, size_t N, int sides, size_t *win);
/* Host rule, no device: the period of every scale, T_s = 2 PI dt scale_s / w0 = 1 / fc_s of tspws_bands_from_frequencies (operations in
 * that order), written to T[S].  A NULL scale / T (with S > 0) and dt or w0 <= 0 (or not finite) return TSPWS_E_ARG. */
int  tspws_ftan_periods(const double *scale, unsigned S, double w0, double dt, double *T);

/* ---- the stack's coherence filter per trace ---- */
/* The rows a dv/v time series is measured on -- one per day, or per short moving stack -- are the noisy ones.  The phase coherence of the
 * whole ensemble is a time-scale filter for each of them (Baig et al. 2009, Hadziioannou et al. 2011, there with the S transform): with Y_i
 * the frame coefficients of target i and W the weight that the stack applies to ST,
 *   x~_i = (float) ICWT(Y_i W_b).
 * Ensemble b is the traces [h_first[b], h_first[b+1]) of d_sigall, M_b of them; u_i is the unit phasor of trace i by the library's rule (a
 * quotient that is no unit phasor adds nothing), PS_b = sum_i u_i.  Stage and counts follow tspws_hip_stack_batch: single-stage K = M_b and
 * PS over the traces; two-stage (0 < Kmax <= M_b) PS over the Kmax partial stacks and K = Kmax.  W is the dimensionless weight per
 * coefficient, the stack's without its ST and 1 / M factors, by the mode of (wu, unbiased, K) as in tspws_hip_weight; every FP64 operation
 * below is rounded on its own (no contraction), in this order:
 *   mode 0 (wu == 2)            g = 1 / (K K);  W = (PS.re PS.re + PS.im PS.im) g
 *   mode 1 (wu == 1)            g = 1 / K;      W = hypot(PS.re, PS.im) g
 *   mode 2 (any other wu)       W = pow(hypot(PS.re, PS.im) / K, wu)
 *   mode 3 (wu == 2, unbiased, K != 1)   iK = 1 / K, iK1 = 1 / (K - 1);  px = PS.re iK, py = PS.im iK;  c = px px + py py;  W = (K c - 1) iK1
 * (mode 3 can be negative, as in the reference) and the filtered coefficient is (Y.re W, Y.im W).  By linearity the mean of an ensemble's
 * filtered traces is its tsPWS row, up to rounding.
 * Leave-one-out (loo == 1, single-stage ensembles only): trace i is filtered with the W of PS_b - u_i (one subtraction per component) and
 * K - 1, mode by K - 1 (K - 1 == 1 falls back to mode 0 by the reference's rule), so that its own phase does not vouch for itself; u_i is
 * what the accumulation added for it -- nothing when the rule skipped it.  An ensemble with M_b < 2 gives NaN rows and counts as left out.
 *
 * tspws_hip_filter_coef: the weight applied to coefficient sets of the caller's.  d_Y is [nrow][ncoef] complex (tspws_hip_forward_f32's
 * layout), h_ens[nrow] names the ensemble of every row (NULL: nrow == B, row i of ensemble i), d_PS is [B][ncoef] complex, h_K[B] the
 * counts; d_out [nrow][ncoef] receives Y W (NULL: in place).  The bits of a row depend on its own set, its ensemble's PS and K and the mode
 * alone, not on nrow, the other rows or how a caller cuts the rows into calls.  NULL d_Y / d_PS / h_K / plan, loo outside {0, 1}, a NaN or
 * infinite wu, a count of 0 (loo: below 2), an h_ens entry >= B (or no h_ens with nrow != B), more than 65535 ensembles and more than
 * 2^32 - 16 rows return TSPWS_E_ARG ("filter_coef: ..."); nrow == 0 or B == 0 returns 0 and does nothing.
 * tspws_hip_filter_traces: the whole call.  `p` must be resolved; wu, unbiased and Kmax are taken from it.  Targets: with d_rows == NULL the
 * ensembles' own traces, and d_out is [h_first[B] - h_first[0]][ldo] floats, row i - h_first[0] being trace i (an empty ensemble writes
 * nothing); else M rows per ensemble, d_rows [B][M][ldr] floats with h_mtr [B][M] host counts as for tspws_hip_stretch_rows (NULL: every
 * row; a count of 0: the row is left out), filtered with the W of the ensemble's traces, and d_out is [B][M][ldo] (rows left out and the
 * rows of an empty ensemble: NaN).  Without d_rows, M must be 0 and h_mtr NULL.  Columns max .. ld-1 are never read, columns max .. ldo-1
 * never written.
 * In rounds of whole ensembles whose blocks stay within TSPWS_PART_MB: the targets' coefficient sets (16 ncoef B a row), the FP64 rows of
 * the inverse, a PS and a W plane per ensemble and one ST plane.  A round is ONE tspws_hip_forward_f32 on its targets, PS per ensemble from
 * tspws_hip_accumulate on the sets just made (trace targets, single-stage), tspws_hip_stacks_float on the ensemble's traces (row targets)
 * or tspws_hip_partial_stacks + tspws_hip_stacks_double (two-stage), the weights, tspws_hip_inverse (ONE call, unless its octave buffer
 * for all the round's rows would exceed the budget: then on as many rows at a time as fit) and the cast.  An ensemble whose
 * blocks alone exceed the budget gets its PS first, chunk by chunk, and its targets are then transformed a second time in chunks.
 * Refusals, TSPWS_E_ARG ("filter_traces: ...") before any device work, outputs untouched, the checks that need no plan first: NULL p /
 * h_first / d_out (d_sigall when there are traces), decreasing offsets, loo outside {0, 1}, d_rows without M, M or h_mtr without d_rows, loo
 * with d_rows, loo with a two-stage ensemble, more than 2^32 - 16 target rows; then a NULL plan and ld, ldr or ldo < max.  B == 0 returns 0
 * and does nothing.  Nothing is atomic, every output has one writer, a repeated call is bit-identical.  The call waits for `stream`: on
 * return the outputs are complete. */
int  tspws_hip_filter_coef(tspws_hip_plan *plan, const double *d_Y, const unsigned *h_ens, size_t nrow, const double *d_PS, const unsigned *h_K,
                           unsigned B, double wu, int unbiased, int loo, double *d_out, void *stream);
int  tspws_hip_filter_traces(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, const size_t *h_first, unsigned B,
                             const float *d_rows, size_t ldr, unsigned M, const unsigned *h_mtr, int loo, float *d_out, size_t ldo, void *stream);
/* How the plan's last tspws_hip_filter_traces / tspws_hip_filter_coef call that did work went (all zero before the first one). */
typedef struct {
	unsigned rounds;       /* rounds of whole ensembles (filter_coef: chunks of rows)                                  */
	unsigned rows;         /* target rows that were filtered                                                           */
	unsigned left_out;     /* rows left out: by h_mtr, of an empty ensemble, or under loo of an ensemble with M_b < 2  */
	unsigned single_stage; /* ensembles with traces, by stage rule ...                                                 */
	unsigned two_stage;
	unsigned empty;        /* ... and those without                                                                    */
	unsigned twice;        /* ensembles whose traces were transformed twice (their blocks alone exceed the budget)     */
} tspws_hip_filter_stats;
int  tspws_hip_filter_traces_stats(const tspws_hip_plan *plan, tspws_hip_filter_stats *stats);

/* ---- convergence curves ------------------------------------------------------------------------ */
/* Similarity / misfit of the stack of the first i+1 traces against a reference, for i = 0..mtr-1
 * (ts_pws1f_lib.c:247-314, similarity :433-449, misfit :452-462).  d_ref_ts / d_ref_ls are [max] floats on the
 * device (the caller passes in->reference for both, or the final tsPWS / ls); the four h_ arrays receive mtr doubles;
 * d_*_steps, when not NULL, receive the [mtr][max] float stacks of every step. */
int  tspws_hip_convergence(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, size_t mtr,
                           const float *d_ref_ts, const float *d_ref_ls, double *h_ts_sim, double *h_ts_misfit,
                           double *h_ls_sim, double *h_ls_misfit, float *d_ts_steps, float *d_ls_steps, void *stream);

/* The convergence curves of B ensembles of one trace array in ONE call.  Ensemble b = the traces [h_first[b], h_first[b+1]) of d_sigall
 * (the rules of tspws_hip_stack_batch: B + 1 non-decreasing host offsets, h_first[0] may be > 0, ld >= max), T = h_first[B] - h_first[0].
 * d_ref_ts / d_ref_ls are [B][max] floats on the device: row b is the reference of ensemble b.  Entry i - h_first[0] of the four host
 * curves ([T] doubles) and row i - h_first[0] of d_ts_steps / d_ls_steps (NULL or [T][max] floats on the device) belong to trace i; the
 * entries of ensemble b are what tspws_hip_convergence gives for that ensemble alone with rows b of the references:
 *   ts-PWS step Tr = j + 1 (j = index inside the ensemble): Kmax == 0 or Tr <= Kmax -- trace j is added to the ensemble's running linear /
 *   phase stacks, weight with K = M = Tr (Tr = 1: the K = 1 rule); otherwise a two-stage stack of the first Tr traces from scratch (row g of
 *   Kmax partial stacks = the FP64 sum, in trace order, of the traces j' < Tr with floor(j' Kmax / Tr) == g; weight with K = Kmax, M = Tr).
 *   Then one inverse, sim = sum d r / sqrt(sum d^2) / sqrt(sum r^2), misfit = sum (d - r)^2 against row b of d_ref_ts, (float) d to d_ts_steps.
 *   linear step: d += x_j; d *= (double)(float)(1.0 / (j + 1)); metrics against row b of d_ref_ls; steps; d *= (j + 1); from zero for every ensemble.
 * An empty ensemble has no entries.  With exactly one non-empty ensemble the call IS tspws_hip_convergence for it.  B == 0 or T == 0: returns 0
 * and does nothing.  A NULL plan, p, h_first, d_sigall, reference or host curve, decreasing offsets or ld < max: TSPWS_E_ARG before any device
 * work, outputs untouched.  Fold and mean removal stay with the caller.  Every sum has a fixed order, nothing is atomic; every scratch block
 * that grows with T stays within TSPWS_PART_MB (rounds).  The call uploads its tables and waits for `stream`: on return the host arrays are
 * filled. */
int  tspws_hip_convergence_batch(tspws_hip_plan *plan, const t_tsPWS *p, const float *d_sigall, size_t ld, const size_t *h_first, unsigned B,
                                 const float *d_ref_ts, const float *d_ref_ls, double *h_ts_sim, double *h_ts_misfit, double *h_ls_sim,
                                 double *h_ls_misfit, float *d_ts_steps, float *d_ls_steps, void *stream);
/* How the plan's last tspws_hip_convergence_batch call with traces went (all zero before the first one). */
typedef struct {
	unsigned single_steps;    /* incremental steps (Tr <= Kmax, or no two-stage rule)                                  */
	unsigned two_stage_steps; /* steps recomputed as two-stage stacks (Tr > Kmax)                                      */
	unsigned rows;            /* partial-stack rows of those steps: Kmax each                                          */
	unsigned rounds;          /* rounds of incremental steps + rounds of two-stage steps (0 when looped)               */
	unsigned looped;          /* 1: the only non-empty ensemble went through tspws_hip_convergence                     */
	unsigned empty;           /* ensembles without traces                                                              */
} tspws_hip_conv_batch_stats;
int  tspws_hip_convergence_batch_stats(const tspws_hip_plan *plan, tspws_hip_conv_batch_stats *stats);

/* ---- several devices of one process (single process, ncclCommInitAll, one stream per device) ---------------
 * Traces shard contiguously by global index; what shards is the sum of partial_linear_stacks (ts_pws1f_lib.c:866-881) --
 * single-stage: of ST || PS (:486-494).  The devices' buffers are added by ONE RCCL all-reduce (fp64, sum) over xGMI.
 * RCCL is bound at run time (librccl.so.1), so single-device users never load it.
 *   TSPWS_COMM=local  own reduction kernel instead of RCCL; also chosen when the device list names a device twice (RCCL
 *                     refuses that) -- lets the N-way bookkeeping run on a one-GPU box; not a fallback: a list with
 *                     DISTINCT devices is refused under it (several physical devices always reduce through RCCL)
 *   TSPWS_COMM=rccl   go through RCCL even for a single device */
typedef struct tspws_hip_comm tspws_hip_comm;
/* communicator over `ndev` devices of this process; devices == NULL: 0 .. ndev-1 */
int   tspws_hip_comm_create(tspws_hip_comm **comm, int ndev, const int *devices);
void  tspws_hip_comm_destroy(tspws_hip_comm *comm);
int   tspws_hip_comm_size(const tspws_hip_comm *comm);
int   tspws_hip_comm_device(const tspws_hip_comm *comm, int i);
void *tspws_hip_comm_stream(const tspws_hip_comm *comm, int i);      /* the communicator's own stream on device i */
const char *tspws_hip_comm_backend(const tspws_hip_comm *comm);      /* "rccl 2.x.y" or "local" */
/* In-place sum: d_bufs[i] = `count` doubles on device i; ordered on streams[i] (NULL array / entry: the communicator's
 * stream of that device).  One ncclAllReduce per device inside ncclGroupStart / ncclGroupEnd. */
int   tspws_hip_allreduce_f64(tspws_hip_comm *comm, double *const *d_bufs, size_t count, void *const *streams);
/* Sum into device `root` only (one ncclReduce per device): the replica rows of a sharded jackknife go to the device that finishes them. */
int   tspws_hip_reduce_f64(tspws_hip_comm *comm, double *const *d_bufs, size_t count, int root, void *const *streams);
/* contiguous shard of `r` of `n`: traces [*first, *first + *count) */
void  tspws_shard_range(size_t mtr, unsigned r, unsigned n, size_t *first, size_t *count);

/* The whole call over trace shards: one plan per device + the communicator.  tspws_main uses it when TSPWS_DEVICES names
 * several devices ("0,1,2,3" or "all").  d_shards[r] = the shard of device r (tspws_shard_range), row stride ld; d_ls /
 * d_tsPWS live on the first device.  The finish stage is split by scales over the devices (tspws_hip_finish_shard) and a
 * second small all-reduce adds the partial reconstructions.  Returns after synchronising the devices. */
typedef struct tspws_hip_multi tspws_hip_multi;
int   tspws_hip_multi_create(tspws_hip_multi **m, int ndev, const int *devices, int type, unsigned J, unsigned V, unsigned N,
                             double s0, double b0, double w0, int uni);
void  tspws_hip_multi_destroy(tspws_hip_multi *m);
tspws_hip_comm *tspws_hip_multi_comm(tspws_hip_multi *m);
tspws_hip_plan *tspws_hip_multi_plan(tspws_hip_multi *m, int i);
/* host traces -> shards (the host array is pinned once, every device pulls its shard on its own stream: all PCIe links at
 * once); *d_shards = per-device buffers owned by m, *d_ls / *d_tsPWS = output buffers on the first device */
int   tspws_hip_multi_upload(tspws_hip_multi *m, const float *h_sigall, size_t ld, size_t mtr, const float *const **d_shards,
                             float **d_ls, float **d_tsPWS);
/* fold / mean removal on the uploaded shards, mirrored back into h_sigall (ts_pws1f_lib.c:71-88, :159-169) */
int   tspws_hip_multi_prologue(tspws_hip_multi *m, float *h_sigall, size_t max, size_t ld, size_t mtr, int fold, int rm);
int   tspws_hip_multi_stack(tspws_hip_multi *m, const t_tsPWS *p, const float *const *d_shards, size_t ld, size_t mtr,
                            float *d_ls, float *d_tsPWS);
/* ... and its C jackknife replicas (two-stage only): one pass per shard, the rows all-reduced, device r finishes replicas
 * [r C / n, (r + 1) C / n) and writes its rows of the HOST arrays h_ls_out / h_ts_out ([C][max] floats). */
int   tspws_hip_multi_stack_jackknife(tspws_hip_multi *m, const t_tsPWS *p, const float *const *d_shards, size_t ld, size_t mtr,
                                      float *d_ls, float *d_tsPWS, const char *h_sel, unsigned C,
                                      float *h_ls_out, float *h_ts_out, unsigned *h_mtr_out);

/* ---- the drop-in on a named device, and its cache -----------------------------------------------------
 * tspws_main (ts_pws1f_lib.h; reference: ts_pws1f_lib.h:104) runs on the device TSPWS_DEVICE names (default 0; a one-entry
 * TSPWS_DEVICES means the same).  tspws_main_on is the same call on an explicit device -- no environment variable is
 * consulted -- for hosts that run one stacking thread per GPU (several station pairs at once): calls on different devices
 * run concurrently, calls on the same device are serialised (per-device lock).
 * Each device keeps the frame and the device trace buffer of its last call for the next one (same parameters: nothing to
 * rebuild; the memory stays allocated between calls).  tspws_main_release frees all of them; TSPWS_PLAN_CACHE=0 in the
 * environment disables the cache altogether.  tspws_main_cached_devices: bit i set = device i holds a cached frame. */
int  tspws_main_on(int device, t_tsPWS *tspws, t_tsPWS_out *out, t_data *in);
void tspws_main_release(void);
unsigned long long tspws_main_cached_devices(void);

/* ---- synthetic ensembles for bench / tests ------------------------------------ */
/* trace i = first+local, sample n: 0.2 sin(2pi(n-N/2)/200) exp(-((n-N/2)/(0.05N))^2/2) + U(-.5,.5) */
int  tspws_hip_synth(float *d_sigall, size_t mtr, size_t N, size_t ld, uint64_t seed, size_t first, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TSPWS_HIP_H */
