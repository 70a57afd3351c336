// What the two trace-form thresholding objectives share (thresh_trace.hip: one scalar pair (u, v) per point; thresh_cols.hip: one
// threshold per factor column): the overflow-free sigmoid, the lane count per point and the k x k Gram pass over the transformed factors.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ void sigmoid_pair_t(double z, double lam, double& s, double& d) {   // (as thresh64.hip)
    if (z >= 0) s = 1.0 / (1.0 + exp(-z));
    else { const double e = exp(z); s = e / (1.0 + e); }
    d = lam * s * (1.0 - s);
}

// S = Us / Vs, D = dUs / dVs: [p][rows_alloc][KC] transformed factors of point p (zero in padding rows and columns).  One block per
// (point, matrix, chunk of 4096 / KC rows): grampart[q][p][chunk][a * KC + b] = sum over the chunk's rows of S[row][a] * D'[row][b],
// D' = S for q = 0 (Us^T Us), 1 (Vs^T Vs) and D' = D for q = 2 (Us^T dUs), 3 (Vs^T dVs; GRAD only).  Rows in order, one accumulator.
template <int KC, bool GRAD>
__global__ __launch_bounds__(256) void trace_gram_kernel(int64_t mrows, int64_t nrows, int npairs_alloc, const double* __restrict__ Us,
                                                          const double* __restrict__ dUs, const double* __restrict__ Vs, const double* __restrict__ dVs,
                                                          double* __restrict__ grampart, int uchunks, int vchunks) {
    constexpr int CR = 4096 / KC;           // rows per chunk
    __shared__ double sh[2 * CR * KC];      // the S and D chunks (64 KiB)
    const int gb = (int)blockIdx.x;
    const int per_pair_blocks = (GRAD ? 2 : 1) * (uchunks + vchunks);
    const int p = gb / per_pair_blocks;
    int r = gb % per_pair_blocks;
    const bool second = r >= uchunks + vchunks;   // the H matrices (S^T D)
    if (second) r -= uchunks + vchunks;
    const bool is_u = r < uchunks;
    const int chunk = is_u ? r : r - uchunks;
    const int64_t ralloc = is_u ? mrows : nrows;
    const double* S = (is_u ? Us : Vs) + (int64_t)p * ralloc * KC;
    const double* D = second ? ((is_u ? dUs : dVs) + (int64_t)p * ralloc * KC) : S;
    const int64_t r0 = (int64_t)chunk * CR;
    const int nr = (int)min((int64_t)CR, ralloc - r0);
    double* sS = sh;
    double* sD = sh + CR * KC;
    for (int e = threadIdx.x; e < CR * KC; e += 256) {
        const bool in = e < nr * KC;
        sS[e] = in ? S[r0 * KC + e] : 0.0;
        sD[e] = in ? D[r0 * KC + e] : 0.0;
    }
    __syncthreads();
    constexpr int EPT = KC * KC / 256;   // elements per thread (KC = 16: one)
    double acc[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) acc[e] = 0.0;
#pragma unroll 8
    for (int row = 0; row < CR; ++row) {   // (unrolled: the LDS reads of eight rows in flight; one accumulator, rows in order)
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int el = threadIdx.x + 256 * e;
            acc[e] = fma(sS[row * KC + el / KC], sD[row * KC + el % KC], acc[e]);
        }
    }
    // grampart[q][p][chunk][KC * KC], q = 0: Us^T Us, 1: Vs^T Vs, 2: Us^T dUs, 3: Vs^T dVs; chunk slots: max(uchunks, vchunks)
    const int qm = (second ? 2 : 0) + (is_u ? 0 : 1);
    const int cmax = uchunks > vchunks ? uchunks : vchunks;
    double* out = grampart + (((int64_t)qm * npairs_alloc + p) * cmax + chunk) * (KC * KC);
#pragma unroll
    for (int e = 0; e < EPT; ++e) out[threadIdx.x + 256 * e] = acc[e];
}

int kc_of(int k) { return k <= 16 ? 16 : (k <= 32 ? 32 : 64); }

}  // namespace
