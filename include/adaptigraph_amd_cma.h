/* adaptigraph_amd_cma.h - C-ABI of the CMA-ES search, gfx950 only.  A library of its own, libadaptigraph_hip_cma.so, beside the
 * engine's (adaptigraph_amd.h): the search needs no engine context - no weights, no workspace - only a device and a stream.
 *   - Every function returns 0 (or a count) on success, a negative AG_ERR_* code of adaptigraph_amd.h otherwise;
 *     ag_cma_last_error returns the calling thread's last message.
 *   - d_* pointers are device memory, h_* host memory; `stream` is a hipStream_t (NULL: the default stream) of `device`.
 *   - The library owns no memory and keeps nothing between calls. */
#ifndef ADAPTIGRAPH_AMD_CMA_H
#define ADAPTIGRAPH_AMD_CMA_H
#include "adaptigraph_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- CMA-ES search: (mu/mu_w, lambda) with positive weights, fp64 (Hansen 2016); no active update, no restarts ----
 *
 * The optimiser the reference runs through the `cma` package (physics_param_optimizer.py:125-175), as three kernels whose
 * generation never waits for the host: sampling from N(m, sigma^2 C), ranking the popsize returned values, recombination, the two
 * evolution paths, the rank-1 / rank-mu covariance update and the matrix square root.  Dimension n, population popsize,
 * mu = popsize / 2, w_i = ln((popsize + 1) / 2) - ln i normalised to sum 1, and mu_eff, c_sigma, d_sigma, c_c, c_1, c_mu, chi_n as
 * in the tutorial's table 1 - computed once, on the host, when the state is filled.
 *
 * THE STATE is one caller-owned device buffer of ag_cma_state_doubles doubles; the library keeps nothing else.  Layout, in doubles:
 *   [0] n  [1] popsize  [2] mu  [3] maximize (0 / 1)  [4] g, generations told  [5] status word  [6] sigma  [7] mu_eff  [8] c_sigma
 *   [9] d_sigma  [10] c_c  [11] c_1  [12] c_mu  [13] chi_n  [14] period  [15] best value so far, as it was given (+inf, or -inf when
 *   maximising, before the first)  [16] the generation g it was sampled in (-1: none)  [17] a mark that the buffer was filled
 *   [18..23] reserved, then from word 24:
 *   m (n) | C (n,n) | p_sigma (n) | p_c (n) | A = C^(1/2) (n,n) | A^-1 (n,n) | scale (n) | lo (n) | hi (n) | periodic (n, 0 / 1) |
 *   best phenotype (n) | weights (mu)
 * m is the GENOTYPE mean; a sample's genotype is m + sigma scale o (A z), its phenotype bound(genotype), per coordinate in fp64: a
 * periodic coordinate is first wrapped into [-period/2, period/2); a coordinate with finite lo < hi is then folded - with
 * w = hi - lo and t = (g - lo) mod 2w in [0, 2w) it becomes lo + (t <= w ? t : 2w - t), a point inside [lo, hi] stays as it is bit
 * for bit - and one with an infinite limit passes through.  The update uses the unfolded steps.  A and A^-1 are the SYMMETRIC roots
 * B diag(sqrt d) B^T and B diag(1 / sqrt d) B^T: they do not depend on the sign or order of the eigenvectors.
 *
 * Status word, sticky until the caller clears it (writes 0 to word 5):
 *   bit 0  fewer than mu of the values told were not NaN: the generation was skipped - every other word of the state is as before,
 *          g included
 *   bit 1  a non-finite number or an eigenvalue <= 0 appeared in the update: it was dropped - every other word is as before
 * Limits: 1 <= n <= 64, 4 <= popsize <= 32768; beyond them ag_cma_state_doubles and ag_cma_init return AG_ERR_UNSUPPORTED with
 * nothing enqueued.  No float atomics; the same inputs give the same bits. */

/* number of doubles of a state, or AG_ERR_UNSUPPORTED */
int ag_cma_state_doubles(int32_t n, int32_t popsize);

/* Fills d_state.  HOST arrays of n: h_x0 the start mean (finite), h_scale > 0 the coordinates' units (sigma is relative to them),
 * h_lo < h_hi the limits (either may be infinite), h_periodic (0 / 1, or NULL for none); sigma0 > 0; period > 0; maximize != 0:
 * larger values are better.  Anything else is AG_ERR_INVALID.  Waits for its one upload (not a per-generation call). */
int ag_cma_init(int32_t device, void* stream, int32_t n, int32_t popsize, const double* h_x0, double sigma0, const double* h_scale,
                const double* h_lo, const double* h_hi, const int32_t* h_periodic, double period, int32_t maximize,
                double* d_state);

/* One population.  d_z (popsize, n) fp64 standard-normal draws (an input, so that a search can be replayed); d_y (popsize, n)
 * fp64 = A z, kept by the caller for the tell; d_x (popsize, n) fp32 phenotypes, each rounded once.  The sizes are read from the
 * state on the device.  Enqueue only. */
int ag_cma_ask(int32_t device, void* stream, const double* d_state, const double* d_z, double* d_y, float* d_x);

/* One update from the fp32 d_values (popsize,) of the population d_y / d_x came from.  Ranking: (value to minimise, index) in
 * lexicographic order - the input negated when maximising; NaN is greater than everything and NaNs are ordered by index; an
 * infinity is a value like any other.  d_order (popsize,) int32: the candidates from best to worst, written even for a skipped
 * generation.  d_improved: one byte, 1 when candidate d_order[0] was strictly better than the best so far (and replaced it), else
 * 0.  The rank-ordered sums are formed in an order that depends on (n, popsize) alone.  Enqueue only. */
int ag_cma_tell(int32_t device, void* stream, double* d_state, const double* d_y, const float* d_x, const float* d_values,
                int32_t* d_order, uint8_t* d_improved);

/* the calling thread's last error message ("" if none) */
const char* ag_cma_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* ADAPTIGRAPH_AMD_CMA_H */
