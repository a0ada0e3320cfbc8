// The CMA-ES search's state layout and launchers (ag_cma.hip).  Internal, not part of the C-ABI.
#pragma once
#include "ag_common.h"

namespace ag {

// ---- CMA-ES search (ag_cma.hip; ag_cma_init / ask / tell).  The whole optimiser state is ONE caller-owned buffer of doubles; its
// layout (include/adaptigraph_amd_cma.h documents it for callers) is a header of CMA_HDR words and then the arrays below.  n and popsize
// are read from the header by the kernels themselves: ask and tell take no sizes, so their launch geometry is fixed.
constexpr int CMA_MAX_N = 64, CMA_MIN_POP = 4, CMA_MAX_POP = 32768, CMA_HDR = 24;
constexpr double CMA_MAGIC = 20231105.0;          // header word CMA_H_MAGIC of a buffer ag_cma_init has filled
enum { CMA_H_N = 0, CMA_H_POP, CMA_H_MU, CMA_H_MAXIMIZE, CMA_H_GEN, CMA_H_STATUS, CMA_H_SIGMA, CMA_H_MUEFF, CMA_H_CS, CMA_H_DS,
       CMA_H_CC, CMA_H_C1, CMA_H_CMU, CMA_H_CHIN, CMA_H_PERIOD, CMA_H_BEST_V, CMA_H_BEST_G, CMA_H_MAGIC };
struct CmaLayout {                                // offsets in doubles
    int n, mu, m, C, ps, pc, A, Ai, scale, lo, hi, periodic, best_x, w, total;
    __host__ __device__ CmaLayout(int n_, int mu_) : n(n_), mu(mu_) {
        m = CMA_HDR; C = m + n; ps = C + n * n; pc = ps + n; A = pc + n; Ai = A + n * n; scale = Ai + n * n; lo = scale + n;
        hi = lo + n; periodic = hi + n; best_x = periodic + n; w = best_x + n; total = w + mu;
    }
};
hipError_t launch_cma_ask(const double* state, const double* z, double* y, float* x, hipStream_t st);
hipError_t launch_cma_tell(double* state, const double* y, const float* x, const float* values, int* order, uint8_t* improved,
                           hipStream_t st);

}  // namespace ag
