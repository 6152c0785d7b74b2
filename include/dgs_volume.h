/*
 * dgs_volume.h -- C ABI of the D = 3 Gaussian sampler, in libdgs.so.
 *
 * Beyond the reference: its device functions have no D = 3 branch (forward.cu:164-275,
 * backward.cu:108-416), its radius is 0 there (forward.cu:52-61) and its sample keys are left
 * uninitialised (sampler_impl.cu:177-182), so at D = 3 it renders nothing.  This path is the
 * reference's per-pair arithmetic carried to three dimensions:
 *   X_d   = mean_d - sample_d, wrapped as forward.cu:149-157 does per axis (period 2; an axis
 *           may be open instead, dgs_volume_preprocess_axes below)
 *   power = -0.5f * (c00 X0 X0 + c11 X1 X1 + c22 X2 X2) - (c01 X0 X1 + c02 X0 X2 + c12 X1 X2),
 *           conics packed [c00 c01 c02 c11 c12 c22] (the reference's D(D+1)/2 row-major
 *           upper triangle, sample_points.cu:40); a pair with power > 0 is skipped
 *   a     = A X;  outputs v G t with G = expf(power) and
 *           gaussian t = 1, derivative t_i = a_i, laplacian t_ij = a_i a_j - A_ij,
 *           third t_ijk = A_ij a_k + A_ik a_j + A_jk a_i - a_i a_j a_k
 *           (the D = 2 expressions of forward.cu:164-275 in index form)
 * summed over EVERY Gaussian (no tile truncation: a pair is left out only when its
 * contribution is exactly 0 in fp32, i.e. X^T A X > 210 for a well-conditioned positive-
 * definite conic; other Gaussians are evaluated against every sample).
 *
 * Same conventions as dgs.h: device pointers, fp32 row-major, asynchronous on `stream`
 * except dgs_volume_preprocess (one host sync), buffers from the caller.
 */
#ifndef DGS_VOLUME_H_INCLUDED
#define DGS_VOLUME_H_INCLUDED

#include "dgs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Binning of a D = 3 field: Gaussians and samples sorted into one uniform grid of cells no
 * smaller than the largest exact-zero cut half-width.  means[P][3], conics[P][6], samples[N][3].
 * The opaque buffer (DGS_BUF_BINNING) is requested through `alloc`; scratch as DGS_BUF_SCRATCH.
 * Synchronises `stream` once (bounds, to size the grid).  forward/backward must be given the
 * same means, conics and samples (re-bin when they change): every forward / backward /
 * count_pairs call compares its tensors bitwise with the binned ones on the device (no sync)
 * and, on a difference, writes NaN to every output, as for a stale buffer (count_pairs
 * returns DGS_ERR_BUFFER).  The buffer holds the flag word these calls reset and set, so the
 * calls on one binning must be ordered (one stream, or events between streams): two
 * concurrent calls could clear each other's flag. */
int dgs_volume_preprocess(int P, int N, const float *means, const float *conics,
                          const float *samples, dgs_alloc_fn alloc, void *alloc_ctx,
                          dgs_stream_t stream, int debug);

/* Open (non-periodic) axes ("Open axes"): the binning with a choice of the wrap per
 * axis, for a time axis or an axis with walls, where a Gaussian near +1 must not reach the samples
 * near -1.  `periodic` is a mask in 0..7, bit d set = axis d periodic; any other value returns
 * DGS_ERR_ARG before any device work.  dgs_volume_preprocess is the periodic = 7 call of this one.
 * On a periodic axis nothing changes.  On an open axis d
 *   X_d = fl(mean_d - sample_d), not wrapped;
 *   only the direct image exists: a pair contributes through its raw distance or not at all;
 *   the coordinates need not lie in [-1, 1]: any finite values are accepted.  In practice keep
 *   |coordinate| below about 100: the cell windows and the cut box test carry an absolute slack of
 *   1e-5, which one fp32 ulp of a coordinate exceeds from about 128 on; beyond that a candidate
 *   exactly on the edge of its cut box (where G is 0 or a subnormal) can be left out, and from
 *   about 1e4 on fp32 no longer resolves the displacements themselves.
 * Everything after X is as above: the power in its stated order without contraction, the
 * power > 0 skip, the exact-zero skip, a = A X, the terms of every function, the classification
 * of the Gaussians and their cut half-widths.  The gradients use the same X (nothing is wrapped
 * on an open axis, so the "wrap with slope 1" does not arise there).
 * The axes are fixed at binning time and stored in the binning buffer: every forward, backward,
 * sample-gradient and count_pairs entry below follows them with an unchanged argument list, and
 * the stale buffer / changed input guard is the same.  A new exported function only:
 * DGS_ABI_VERSION is unchanged. */
int dgs_volume_preprocess_axes(int periodic, int P, int N, const float *means, const float *conics,
                               const float *samples, dgs_alloc_fn alloc, void *alloc_ctx,
                               dgs_stream_t stream, int debug);

/* Workspace bytes of dgs_volume_backward (0 for the forward). */
size_t dgs_volume_workspace_size(int function, int P, int N, int C, int backward);

/* out[N][3^function][C] (every entry written; symmetric entries repeated, as the reference's
 * D = 2 outputs are). */
int dgs_volume_forward(int function, int P, int N, int C, const float *means, const float *values,
                       const float *conics, const float *samples, const void *binning,
                       size_t binning_bytes, float *out, dgs_stream_t stream, int debug);

/* dL_dout[N][3^function][C]; writes (overwrites) dL_dmeans[P][3], dL_dvalues[P][C],
 * dL_dconics[P][6]. */
int dgs_volume_backward(int function, int P, int N, int C, const float *means, const float *values,
                        const float *conics, const float *samples, const float *dL_dout,
                        const void *binning, size_t binning_bytes, float *dL_dmeans,
                        float *dL_dvalues, float *dL_dconics, void *workspace,
                        size_t workspace_bytes, dgs_stream_t stream, int debug);

/* Fused functions (the D = 3 form of dgs_sample_*_multi in dgs.h): one walk of the candidates
 * for every function of `mask` (bit f set = function f, mask in 1..15; DGS_ERR_ARG otherwise),
 * as a PDE residual needs several of the four at the same points per step.
 *   forward : outs[f] = out of function f (as dgs_volume_forward, every entry written), for
 *             every f in mask; the other entries are ignored and may be NULL.  Each output is
 *             bit-identical to dgs_volume_forward's (the same addends in the same order).
 *   backward: dL_douts[f] = dL/d out of function f for every f in mask; writes (overwrites)
 *             the gradients of the summed loss, sum_f <dL_douts[f], out_f>, with no atomics
 *             (repeated calls are bit-identical).
 * Two or more functions need C = 1 (DGS_ERR_ARG otherwise: call the per-function entry points
 * and add their gradients); a single-bit mask is the per-function path for any C, and its
 * workspace size is dgs_volume_workspace_size's.  Backward workspace of a multi-bit mask:
 * N * (unique components of the mask's functions: 1 + 3 + 6 + 10 for all four) * 4 bytes; the
 * forward needs none.  A missing or short binning gives DGS_ERR_BUFFER.  Edge sizes, the stale
 * buffer / changed input guard (NaN in every output or gradient) and the ordering of calls on
 * one binning are those of the per-function calls; no host sync, no allocation. */
size_t dgs_volume_workspace_size_multi(int mask, int P, int N, int C, int backward);
int dgs_volume_forward_multi(int mask, int P, int N, int C, const float *means, const float *values,
                             const float *conics, const float *samples, const void *binning,
                             size_t binning_bytes, float *const *outs, dgs_stream_t stream, int debug);
int dgs_volume_backward_multi(int mask, int P, int N, int C, const float *means, const float *values,
                              const float *conics, const float *samples, const float *const *dL_douts,
                              const void *binning, size_t binning_bytes, float *dL_dmeans,
                              float *dL_dvalues, float *dL_dconics, void *workspace,
                              size_t workspace_bytes, dgs_stream_t stream, int debug);

/* Gradient with respect to the sample positions (DESIGN.md §4.9, D = 3).  `mask` and dL_douts are
 * those of dgs_volume_backward_multi (a single function f is the mask 1 << f, any C; two or more
 * functions need C = 1, DGS_ERR_ARG otherwise).  Writes (overwrites) dL_dsamples[N][3]:
 *   dL/ds_n = sum_g G (phi a - A g),  phi = sum_u hv_u t_u,  g = d phi / d a,
 *   hv_u = sum_ch v_ch h_u,ch,  h = dL summed over the full components of unique component u,
 * summed over the forward's pair set (the pair set held fixed, the wrap with slope 1); per pair it
 * is minus that pair's share of dL_dmeans, so sum_n dL/ds_n = -sum_p dL/dm_p.  One walk of the
 * candidates, lane = sample, no atomics (repeated calls are bit-identical).  Zeros for P = 0,
 * nothing to do for N = 0; the stale buffer / changed input guard writes NaN to every entry.  No
 * host sync, no allocation; calls on one binning are ordered as the others are.  The workspace
 * size is 0 today (workspace may be NULL); callers size it through the function all the same.
 * New exported functions only: DGS_ABI_VERSION is unchanged (dgs.h, on the D = 2 pair). */
size_t dgs_volume_sample_grad_workspace_size(int mask, int P, int N, int C);
int dgs_volume_backward_samples(int mask, int P, int N, int C, const float *means, const float *values,
                                const float *conics, const float *samples, const float *const *dL_douts,
                                const void *binning, size_t binning_bytes, float *dL_dsamples,
                                void *workspace, size_t workspace_bytes, dgs_stream_t stream, int debug);

/* Fused functions of a multi-channel field: the *_multi / *_samples calls above with one walk of
 * the candidates also for two or more functions at 2 <= C <= DGS_VOLUME_FUSED_MAX_C (a velocity
 * field, C = 3, or velocity and pressure, C = 4).  Same argument lists.
 *   - a single-bit mask (any C) or C = 1 (any mask): the call is dgs_volume_forward_multi /
 *     dgs_volume_backward_multi / dgs_volume_backward_samples itself, the same checks, the same
 *     launches, bit-identical results;
 *   - two or more functions at 2 <= C <= DGS_VOLUME_FUSED_MAX_C: one walk for every function and
 *     every channel.  outs[f] / dL_douts[f] are [N][3^f][C].  Each output is bit-identical to
 *     dgs_volume_forward's and does not depend on the other functions of the mask; the gradients
 *     equal the sum of the per-function calls' to rounding (another order of the same sums), with
 *     no atomics, so repeated calls are bit-identical.  Backward workspace: N * (unique components
 *     of the mask's functions) * C * 4 bytes; the forward and the sample gradient need none;
 *   - two or more functions above the limit: DGS_ERR_ARG (call the per-function entry points and
 *     add), and the workspace size is 0.
 * Edge sizes, the stale buffer / changed input guard (NaN in every output of the mask, every
 * gradient and dL_dsamples), DGS_ERR_BUFFER for a missing or short binning and the ordering of
 * calls on one binning are those of the calls above; no host sync, no allocation.  New exported
 * functions only: DGS_ABI_VERSION is unchanged. */
#define DGS_VOLUME_FUSED_MAX_C 4
size_t dgs_volume_workspace_size_fused(int mask, int P, int N, int C, int backward);
int dgs_volume_forward_fused(int mask, int P, int N, int C, const float *means, const float *values,
                             const float *conics, const float *samples, const void *binning,
                             size_t binning_bytes, float *const *outs, dgs_stream_t stream, int debug);
int dgs_volume_backward_fused(int mask, int P, int N, int C, const float *means, const float *values,
                              const float *conics, const float *samples, const float *const *dL_douts,
                              const void *binning, size_t binning_bytes, float *dL_dmeans,
                              float *dL_dvalues, float *dL_dconics, void *workspace,
                              size_t workspace_bytes, dgs_stream_t stream, int debug);
int dgs_volume_backward_samples_fused(int mask, int P, int N, int C, const float *means, const float *values,
                                      const float *conics, const float *samples, const float *const *dL_douts,
                                      const void *binning, size_t binning_bytes, float *dL_dsamples,
                                      void *workspace, size_t workspace_bytes, dgs_stream_t stream, int debug);

/* A fifth function, the trace of the laplacian (what diffusion, Poisson, wave and Navier-Stokes
 * residuals use of the Hessian; DESIGN.md §4.8, "Trace Laplacian"): code 4, bit 4 of a mask,
 *   out[N][C],  out[n][ch] = sum_g v_g,ch G t,   t = (a0 a0 + a1 a1 + a2 a2) - (c00 + c11 + c22),
 * t evaluated in fp32 in exactly that order without contraction, over the pair set, wrap and
 * exact-zero skip of the other four.  In the gradients it is the laplacian with the sample's
 * tensor H = h I: phi = h t, d phi / d a = 2 h a, d phi / d c = -h on the three diagonal entries.
 * It rounds differently from the sum of the laplacian's three diagonal outputs and is not bitwise
 * that sum.  The forward sum is written out: among the binned Gaussians fma(round(v G), t, acc);
 * among the others round(acc + round(round(v G) t)) at C = 1 and the same fma at C > 1.  So an
 * output of a mask with the trace is bit-identical to the mask-16 call's at the same C.
 *
 * The *_ops entries take the argument lists of the *_fused entries with outs / dL_douts arrays of
 * FIVE pointers (indexed by function code; entries outside the mask ignored).  Valid masks are
 * 1..31 without both bit 2 and bit 4 (the laplacian already holds its trace); DGS_ERR_ARG otherwise.
 *   - mask < 16: the call is the *_fused entry itself (the same checks, the same launches,
 *     bit-identical results; the fifth pointer is not read);
 *   - mask 16: any C (C > 1 in channel blocks of 4 and 8, as the gaussian);
 *   - the trace with some of functions 0, 1, 3 (masks 17, 18, 19, 24, 25, 26, 27): one walk of the
 *     candidates at 1 <= C <= DGS_VOLUME_FUSED_MAX_C; above it DGS_ERR_ARG (call per function and
 *     add) and a workspace size of 0.
 * Backward workspace: N * (unique components of the mask, 1 for the trace) * C * 4 bytes; the
 * forward and the sample gradient need none.  Edge sizes, the stale buffer / changed input guard
 * (NaN in every output of the mask, every gradient and dL_dsamples), DGS_ERR_BUFFER for a missing
 * or short binning and the ordering of calls on one binning are those of the *_fused calls; no
 * host sync, no allocation.  New exported functions only: DGS_ABI_VERSION is unchanged, and the
 * entries above keep refusing bit 4. */
#define DGS_VOLUME_FN_LAPLACIAN_TRACE 4
size_t dgs_volume_workspace_size_ops(int mask, int P, int N, int C, int backward);
int dgs_volume_forward_ops(int mask, int P, int N, int C, const float *means, const float *values,
                           const float *conics, const float *samples, const void *binning,
                           size_t binning_bytes, float *const *outs, dgs_stream_t stream, int debug);
int dgs_volume_backward_ops(int mask, int P, int N, int C, const float *means, const float *values,
                            const float *conics, const float *samples, const float *const *dL_douts,
                            const void *binning, size_t binning_bytes, float *dL_dmeans,
                            float *dL_dvalues, float *dL_dconics, void *workspace,
                            size_t workspace_bytes, dgs_stream_t stream, int debug);
int dgs_volume_backward_samples_ops(int mask, int P, int N, int C, const float *means, const float *values,
                                    const float *conics, const float *samples, const float *const *dL_douts,
                                    const void *binning, size_t binning_bytes, float *dL_dsamples,
                                    void *workspace, size_t workspace_bytes, dgs_stream_t stream, int debug);

/* A sixth function, a constant-coefficient linear operator of the field ("Linear
 * operator"): code 5, bit 5 of a mask,
 *   L u = c0 u + sum_i b_i d_i u + sum_ij W_ij d_ij u,   W symmetric,
 *   coef[10] = [c0, b0, b1, b2, w00, w01, w02, w11, w12, w22]   (w packed like a conic, w_ij the
 *   entry of W; an off-diagonal entry counts twice in W:H),
 *   out[N][C],  out[n][ch] = sum_g v_g,ch G t,
 * over the pair set, wrap and exact-zero skip of the other functions.  With k_u = m_u w_u (m_u = 1
 * on the diagonal, 2 off it, formed on the host, exact) t is evaluated in fp32 without contraction
 * in exactly this order, every sum left to right:
 *   lin = b0 a0 + b1 a1 + b2 a2
 *   q   = k00 (a0 a0 - c00) + k01 (a0 a1 - c01) + k02 (a0 a2 - c02)
 *       + k11 (a1 a1 - c11) + k12 (a1 a2 - c12) + k22 (a2 a2 - c22)
 *   t   = (c0 + lin) + q
 * By definition the output is c0 gaussian + sum_i b_i derivative[i] + sum_ij W_ij laplacian[i][j]
 * of this library's own outputs, with their sign conventions; it rounds differently and is not
 * bitwise that combination.  In the gradients phi = h t, d phi / d a_i = h (b_i + 2 sum_j W_ij a_j),
 * d phi / d c_u = -h k_u.  The forward sum is written out as the trace's: among the binned
 * Gaussians fma(round(v G), t, acc); among the others round(acc + round(round(v G) t)) at C = 1
 * and the same fma at C > 1.  So an output of a mask with the operator is bit-identical to the
 * mask-32 call's at the same C.
 *
 * The coefficients are constants of one call: coef is a HOST pointer to ten floats, read during the
 * call and not needed afterwards; they reach the kernels as launch arguments, so two calls on one
 * binning with different coefficients each see their own.  There is no gradient with respect to
 * them.
 *
 * The *_linop entries take the argument lists of the *_ops entries after (mask, coef), with outs /
 * dL_douts arrays of SIX pointers (indexed by function code; entries outside the mask ignored).
 * Valid masks are 1..63; bit 5 excludes bits 2, 3 and 4 (DGS_ERR_ARG, "mask", otherwise).
 *   - mask < 32: the call is the *_ops entry itself (the same checks, the same launches,
 *     bit-identical results; coef may be NULL and the sixth pointer is not read);
 *   - mask 32: any C (C > 1 in channel blocks of 4 and 8, as the trace);
 *   - the operator with the gaussian and / or the derivative (masks 33, 34, 35): one walk of the
 *     candidates at 1 <= C <= DGS_VOLUME_FUSED_MAX_C; above it DGS_ERR_ARG (call per function and
 *     add) and a workspace size of 0;
 *   - bit 5 with a NULL coef or a non-finite coefficient: DGS_ERR_ARG ("coef") before any device
 *     work.
 * Backward workspace: N * (unique components of the mask, 1 for the operator) * C * 4 bytes; the
 * forward and the sample gradient need none.  Edge sizes, the stale buffer / changed input guard,
 * DGS_ERR_BUFFER for a missing or short binning and the ordering of calls on one binning are those
 * of the *_ops calls; no atomics, no host sync, no allocation.  New exported functions only:
 * DGS_ABI_VERSION is unchanged, and the entries above keep refusing bit 5. */
#define DGS_VOLUME_FN_OPERATOR 5
size_t dgs_volume_workspace_size_linop(int mask, int P, int N, int C, int backward);
int dgs_volume_forward_linop(int mask, const float *coef, int P, int N, int C, const float *means,
                             const float *values, const float *conics, const float *samples,
                             const void *binning, size_t binning_bytes, float *const *outs,
                             dgs_stream_t stream, int debug);
int dgs_volume_backward_linop(int mask, const float *coef, int P, int N, int C, const float *means,
                              const float *values, const float *conics, const float *samples,
                              const float *const *dL_douts, const void *binning, size_t binning_bytes,
                              float *dL_dmeans, float *dL_dvalues, float *dL_dconics, void *workspace,
                              size_t workspace_bytes, dgs_stream_t stream, int debug);
int dgs_volume_backward_samples_linop(int mask, const float *coef, int P, int N, int C, const float *means,
                                      const float *values, const float *conics, const float *samples,
                                      const float *const *dL_douts, const void *binning,
                                      size_t binning_bytes, float *dL_dsamples, void *workspace,
                                      size_t workspace_bytes, dgs_stream_t stream, int debug);

/* Diagnostic (not on any reference API): counts[0] = pairs the forward evaluates (candidates
 * inside their own cut box), counts[1] = live pairs (G = expf(power) > 0).  Host, syncs;
 * DGS_ERR_BUFFER when the inputs differ from the binned ones. */
int dgs_volume_count_pairs(int P, int N, const float *means, const float *conics, const float *samples,
                           const void *binning, size_t binning_bytes, int64_t *counts, dgs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DGS_VOLUME_H_INCLUDED */
