// C-ABI of the CMA-ES search (ag_cma.hip; include/adaptigraph_amd_cma.h): the state's size, its initial contents, ask and tell -
// libadaptigraph_hip_cma.so, a library of its own beside the engine's: it needs no engine context.  The state is the caller's
// buffer; the library keeps nothing between calls but the calling thread's last error message.
#include "../../include/adaptigraph_amd_cma.h"
#include "ag_cma.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

using namespace ag;

namespace {
thread_local std::string cma_err;
int cma_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    cma_err = buf;
    return code;
}
#define CMA_HIPCHK(expr)                                                                                  \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) return cma_fail(AG_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)
}  // namespace

extern "C" {

const char* ag_cma_last_error(void) { return cma_err.c_str(); }

int ag_cma_state_doubles(int32_t n, int32_t popsize) {
    if (n < 1 || n > CMA_MAX_N || popsize < CMA_MIN_POP || popsize > CMA_MAX_POP) return AG_ERR_UNSUPPORTED;
    return CmaLayout(n, popsize / 2).total;
}

int ag_cma_init(int32_t device, void* stream, int32_t n, int32_t popsize, const double* h_x0, double sigma0, const double* h_scale,
                const double* h_lo, const double* h_hi, const int32_t* h_periodic, double period, int32_t maximize, double* d_state) {
    if (n < 1 || n > CMA_MAX_N || popsize < CMA_MIN_POP || popsize > CMA_MAX_POP)
        return cma_fail(AG_ERR_UNSUPPORTED, "ag_cma_init: n = %d, popsize = %d outside 1 <= n <= %d, %d <= popsize <= %d", n, popsize,
                    CMA_MAX_N, CMA_MIN_POP, CMA_MAX_POP);
    if (!h_x0 || !h_scale || !h_lo || !h_hi || !d_state || !(sigma0 > 0.0) || !std::isfinite(sigma0) || !(period > 0.0) ||
        !std::isfinite(period))
        return cma_fail(AG_ERR_INVALID, "ag_cma_init: bad arguments (sigma0 = %g, period = %g)", sigma0, period);
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(h_x0[i]) || !(h_scale[i] > 0.0) || !std::isfinite(h_scale[i]) || std::isnan(h_lo[i]) || std::isnan(h_hi[i]) ||
            !(h_lo[i] < h_hi[i]))
            return cma_fail(AG_ERR_INVALID, "ag_cma_init: coordinate %d: x0 = %g, scale = %g, limits [%g, %g]", i, h_x0[i], h_scale[i],
                        h_lo[i], h_hi[i]);
    }
    // the strategy constants, once, in fp64 (Hansen 2016, table 1; positive weights only)
    const int mu = popsize / 2;
    const CmaLayout L(n, mu);
    std::vector<double> s((size_t)L.total, 0.0);
    double wsum = 0.0, w2 = 0.0;
    for (int i = 0; i < mu; ++i) { s[L.w + i] = std::log((popsize + 1) / 2.0) - std::log((double)(i + 1)); wsum += s[L.w + i]; }
    for (int i = 0; i < mu; ++i) { s[L.w + i] /= wsum; w2 += s[L.w + i] * s[L.w + i]; }
    const double N = n, mueff = 1.0 / w2;
    const double cs = (mueff + 2.0) / (N + mueff + 5.0);
    const double c1 = 2.0 / ((N + 1.3) * (N + 1.3) + mueff);
    s[CMA_H_N] = n; s[CMA_H_POP] = popsize; s[CMA_H_MU] = mu; s[CMA_H_MAXIMIZE] = maximize ? 1.0 : 0.0;
    s[CMA_H_GEN] = 0.0; s[CMA_H_STATUS] = 0.0; s[CMA_H_SIGMA] = sigma0; s[CMA_H_MUEFF] = mueff; s[CMA_H_CS] = cs;
    s[CMA_H_DS] = 1.0 + 2.0 * std::max(0.0, std::sqrt((mueff - 1.0) / (N + 1.0)) - 1.0) + cs;
    s[CMA_H_CC] = (4.0 + mueff / N) / (N + 4.0 + 2.0 * mueff / N);
    s[CMA_H_C1] = c1;
    s[CMA_H_CMU] = std::min(1.0 - c1, 2.0 * (mueff - 2.0 + 1.0 / mueff) / ((N + 2.0) * (N + 2.0) + mueff));
    s[CMA_H_CHIN] = std::sqrt(N) * (1.0 - 1.0 / (4.0 * N) + 1.0 / (21.0 * N * N));
    s[CMA_H_PERIOD] = period;
    s[CMA_H_BEST_V] = maximize ? -INFINITY : INFINITY;
    s[CMA_H_BEST_G] = -1.0;
    s[CMA_H_MAGIC] = CMA_MAGIC;
    for (int i = 0; i < n; ++i) {
        s[L.m + i] = h_x0[i]; s[L.scale + i] = h_scale[i]; s[L.lo + i] = h_lo[i]; s[L.hi + i] = h_hi[i];
        s[L.periodic + i] = h_periodic && h_periodic[i] ? 1.0 : 0.0;
        s[L.C + i * n + i] = s[L.A + i * n + i] = s[L.Ai + i * n + i] = 1.0;
    }
    CMA_HIPCHK(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    CMA_HIPCHK(hipMemcpyAsync(d_state, s.data(), s.size() * sizeof(double), hipMemcpyHostToDevice, st));
    CMA_HIPCHK(hipStreamSynchronize(st));                       // the host vector dies with this call; init is not the hot path
    return AG_OK;
}

int ag_cma_ask(int32_t device, void* stream, const double* d_state, const double* d_z, double* d_y, float* d_x) {
    if (!d_state || !d_z || !d_y || !d_x) return cma_fail(AG_ERR_INVALID, "ag_cma_ask: bad arguments");
    CMA_HIPCHK(hipSetDevice(device));
    CMA_HIPCHK(launch_cma_ask(d_state, d_z, d_y, d_x, static_cast<hipStream_t>(stream)));
    return AG_OK;
}

int ag_cma_tell(int32_t device, void* stream, double* d_state, const double* d_y, const float* d_x, const float* d_values,
                int32_t* d_order, uint8_t* d_improved) {
    if (!d_state || !d_y || !d_x || !d_values || !d_order || !d_improved) return cma_fail(AG_ERR_INVALID, "ag_cma_tell: bad arguments");
    CMA_HIPCHK(hipSetDevice(device));
    CMA_HIPCHK(launch_cma_tell(d_state, d_y, d_x, d_values, d_order, d_improved, static_cast<hipStream_t>(stream)));
    return AG_OK;
}

}  // extern "C"
