// The thresholding objective of BinaryMFThresholdExColumnwise -- one threshold PER FACTOR COLUMN -- for the all-ones mask in TRACE form,
// for a BATCH of points x = [us_0 .. us_{k-1}, vs_0 .. vs_{k-1}] (the candidates of one Wolfe search, solvers/line_search.py).
//
//   Us[i][c] = sigmoid(lamda (U[i][c] - us[c])), dUs = lamda Us (1 - Us), likewise Vs, dVs with vs
//   A0[c] = sum_{X_ij = 1} Us[i][c] Vs[j][c],   A1[c] = sum_{X_ij = 1} dUs[i][c] Vs[j][c],   A2[c] = sum_{X_ij = 1} Us[i][c] dVs[j][c]
//   GU = Us^T Us, GV = Vs^T Vs, HU[c][c'] = sum_i dUs[i][c] Us[i][c'], HV likewise
//   2 F      = sum X - 2 sum_c A0[c] + sum_{c, c'} GU[c][c'] GV[c][c']
//   dF[c]    = A1[c] - sum_c' HU[c][c'] GV[c'][c]            (the scalar model's sign convention, thresh_trace.hip)
//   dF[k+c]  = A2[c] - sum_c' HV[c][c'] GU[c'][c]
//
// The scalar form (thresh_trace.hip) adds the per-cell dot products over the columns before it stores anything; here the sums stay
// apart per column -- 2 k gradient components per point -- and the Gram terms are contracted row by row instead of to a scalar.
// The lane layout of the cell pass is the scalar form's (lane (pl, c) owns column c of point pl), so the three per-column sums are
// already in the lane's registers; a workgroup walks a fixed, strided set of segments and leaves ONE partial per (point, kind,
// column), the partials are added in block order.  fp64 throughout, every sum in a fixed order, no floating-point atomics.
#include "common.h"
#include "trace_gram.h"

#define BMF_COLS_MAX_GROUPS 8
#define BMF_COLS_MAX_SEGMENTS(m) ((int64_t)8 * (m) + 64)   // as bmf_thresh_trace64
#define BMF_COLS_CELL_BLOCKS 512                           // workgroups of the cell pass (two per compute unit), at most
#define BMF_COLS_STAGE 1024                                // doubles of the staged points: pa * 2 * kc is 1024 at every kc

namespace {

// xs[p][h][c], h = 0: us, 1: vs, c < kc: the points as the transform reads them (x may sit in pinned host memory: it is read once,
// here).  Padding points repeat the last real one (their results are never read), padding columns hold 0 (never read).
__global__ __launch_bounds__(1024) void cols_stage_kernel(const double* __restrict__ x, int n_points, int k, int kc, int pa, double* __restrict__ xs) {
    const int t = (int)threadIdx.x;
    if (t >= pa * 2 * kc) return;
    const int p = t / (2 * kc), h = (t / kc) & 1, c = t % kc;
    const int q = p < n_points ? p : n_points - 1;
    xs[t] = c < k ? x[(int64_t)q * 2 * k + h * k + c] : 0.0;
}

// S[p][row][c], c < kc: the factor transformed with point p's threshold of column c (zero for padding rows / columns; one extra
// all-zero row `rows_alloc - 1` that the cell pass points missing cells at).  Blocks [0, gu) of a point do U, the rest V.
__global__ __launch_bounds__(256) void cols_transform_kernel(const double* __restrict__ U, int64_t ldu, int m, int64_t mrows, const double* __restrict__ V,
                                                              int n, int64_t nrows, int k, int kshift, double lam, const double* __restrict__ xs,
                                                              double* __restrict__ Us, double* __restrict__ dUs, double* __restrict__ Vs,
                                                              double* __restrict__ dVs, int gu) {
    const bool is_u = (int)blockIdx.x < gu;
    const int p = (int)blockIdx.y;
    const double* F = is_u ? U : V;
    const int rows = is_u ? m : n;
    const int per_point = (int)((is_u ? mrows : nrows) << kshift);   // < 2^31: checked by the launcher
    double* S = (is_u ? Us : Vs) + (int64_t)p * per_point;
    double* D = (is_u ? dUs : dVs);
    if (D) D += (int64_t)p * per_point;
    const double* thr = xs + ((int64_t)(2 * p + (is_u ? 0 : 1)) << kshift);
    const int b = is_u ? (int)blockIdx.x : (int)blockIdx.x - gu, nb = is_u ? gu : (int)gridDim.x - gu;
    for (int i = b * 256 + (int)threadIdx.x; i < per_point; i += nb * 256) {
        const int r = i >> kshift, c = i & ((1 << kshift) - 1);
        double s_ = 0.0, d_ = 0.0;
        if (r < rows && c < k) sigmoid_pair_t((F[(int64_t)r * ldu + c] - thr[c]) * lam, lam, s_, d_);
        S[i] = s_;
        if (D) D[i] = d_;
    }
}

// The ONES of X, cut into SEGMENTS of at most 128 cells of one row (as bmf_thresh_trace64).  Wave w of block b takes the segments
// 4 b + w, 4 b + w + 4 gridDim.x, ...: lane (pl, c), pl = lane / KC, serves column c of points g * PPI + pl, g < G <= GMAX, and keeps
// its three sums over ALL its segments.  The four waves of a block are added in wave order through the LDS:
// cellpart[p][block][kind][c], kind = 0: A0, 1: A1, 2: A2 (GRAD).  nbmax: block slots per point.
template <int KC, bool GRAD, int GMAX>
__global__ __launch_bounds__(256) void cols_cells_kernel(const int32_t* __restrict__ seg_row, const int64_t* __restrict__ seg_beg,
                                                          const int32_t* __restrict__ seg_len, const int32_t* __restrict__ idx, int nseg,
                                                          int64_t mrows, int64_t nrows, int G, const double* __restrict__ Us,
                                                          const double* __restrict__ dUs, const double* __restrict__ Vs, const double* __restrict__ dVs,
                                                          double* __restrict__ cellpart, int nbmax) {
    constexpr int PPI = 64 / KC;
    constexpr int T = (GRAD ? 16 : 32) / GMAX;   // cells per trip
    constexpr int NV = GRAD ? 3 : 1;
    __shared__ double sh[4][GMAX][NV][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pl = lane / KC, c = lane % KC;
    const int64_t upair = mrows * KC, vpair = nrows * KC;
    const int zrow = (int)(nrows - 1);   // all-zero row
    const double* vlane = Vs + (int64_t)pl * vpair + c;
    const double* dlane = dVs + (int64_t)pl * vpair + c;
    double a0[GMAX], a1[GMAX], a2[GMAX];
#pragma unroll
    for (int g = 0; g < GMAX; ++g) a0[g] = a1[g] = a2[g] = 0.0;
    for (int sg = (int)blockIdx.x * 4 + wave; sg < nseg; sg += (int)gridDim.x * 4) {
        const int i = seg_row[sg];
        const int64_t w0 = seg_beg[sg];
        const int len = seg_len[sg];   // <= 128
        double us[GMAX], dus[GMAX];
#pragma unroll
        for (int g = 0; g < GMAX; ++g) {
            const int64_t p = g * PPI + pl;
            us[g] = g < G ? Us[p * upair + (int64_t)i * KC + c] : 0.0;
            dus[g] = (GRAD && g < G) ? dUs[p * upair + (int64_t)i * KC + c] : 0.0;
        }
        const int myj0 = lane < len ? idx[w0 + lane] : zrow;
        const int myj1 = 64 + lane < len ? idx[w0 + 64 + lane] : zrow;
        for (int st = 0; st < len; st += 64) {
            const int myj = st == 0 ? myj0 : myj1;
            const int nst = min(64, len - st);
            for (int t0 = 0; t0 < nst; t0 += T) {
                double vv[T][GMAX], dv[T][GMAX];
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const int64_t jo = (int64_t)__builtin_amdgcn_readlane(myj, t0 + t) * KC;   // (t0 + t < 64: T divides 64)
#pragma unroll
                    for (int g = 0; g < GMAX; ++g)
                        if (g < G) {
                            vv[t][g] = vlane[(int64_t)(g * PPI) * vpair + jo];
                            if (GRAD) dv[t][g] = dlane[(int64_t)(g * PPI) * vpair + jo];
                        }
                }
#pragma unroll
                for (int t = 0; t < T; ++t)
#pragma unroll
                    for (int g = 0; g < GMAX; ++g)
                        if (g < G) {
                            a0[g] = fma(us[g], vv[t][g], a0[g]);
                            if (GRAD) {
                                a1[g] = fma(dus[g], vv[t][g], a1[g]);
                                a2[g] = fma(us[g], dv[t][g], a2[g]);
                            }
                        }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < GMAX; ++g) {
        sh[wave][g][0][lane] = a0[g];
        if constexpr (GRAD) { sh[wave][g][1][lane] = a1[g]; sh[wave][g][2][lane] = a2[g]; }
    }
    __syncthreads();
    for (int e = (int)threadIdx.x; e < GMAX * NV * 64; e += 256) {
        const int g = e / (NV * 64), kind = (e / 64) % NV, ln = e % 64;
        if (g < G) {
            const int64_t p = g * PPI + ln / KC;
            cellpart[((p * nbmax + (int)blockIdx.x) * 3 + kind) * KC + ln % KC] = ((sh[0][g][kind][ln] + sh[1][g][kind][ln]) + sh[2][g][kind][ln]) + sh[3][g][kind][ln];
        }
    }
}

// One block of 1024 threads per point: the ordered sums, the row-wise contractions of the Gram terms, and the record
// out[p (2 + 2 k) + ...] = (seq, 2 F, dF[0 .. 2 k)) in pinned host memory, with the output protocol of bmf_thresh_trace64: the stamp of
// a point is written behind its values and a system-scope fence (one wave writes the whole record, so the fence covers all of it),
// the LAST block to finish (a device counter) writes the sequence word behind the last record.
template <int KC>
__global__ __launch_bounds__(1024) void cols_final_kernel(const double* __restrict__ cellpart, const double* __restrict__ grampart, int nb, int nbmax,
                                                           int npoints, int npoints_alloc, int uchunks, int vchunks, int k, double sum_x, int want_grad,
                                                           double* __restrict__ out, double seq, unsigned* __restrict__ counter) {
    constexpr int NI = 3 * KC;            // (kind, column) items of the cell sums
    constexpr int NPART = 1024 / NI;      // threads per item: each sums a contiguous run of blocks, the runs are added in order
    constexpr int E = KC * KC;
    __shared__ double sh[3][1024];
    __shared__ double A[NI], col[2][KC];
    const int p = (int)blockIdx.x, t = (int)threadIdx.x;
    // A0, A1, A2 per column: the block partials in block order
    if (t < NPART * NI) {
        const int item = t % NI, part = t / NI;
        double s = 0.0;
        if (want_grad || item < KC) {
            const double* cp = cellpart + (int64_t)p * nbmax * NI + item;
            const int b1 = (int)(((int64_t)nb * (part + 1)) / NPART);
            for (int b = (int)(((int64_t)nb * part) / NPART); b < b1; ++b) s += cp[(int64_t)b * NI];
        }
        sh[0][t] = s;
    }
    __syncthreads();
    if (t < NI) {
        double s = 0.0;
        for (int part = 0; part < NPART; ++part) s += sh[0][part * NI + t];
        A[t] = s;
    }
    __syncthreads();
    // element el = a * KC + b of a Gram matrix: its chunks in order.  < GU, GV > for F; the gradient wants, per column c = el % KC, the sum
    // over a of (Us^T dUs)[a][c] GV[a][c] -- thread t meets the elements t, t + 1024, ... (a ascending, the same c: KC divides 1024)
    const int cmax = uchunks > vchunks ? uchunks : vchunks;
    auto gel = [&](int q, int el) {
        const int nch = (q & 1) ? vchunks : uchunks;
        const double* g = grampart + ((int64_t)q * npoints_alloc + p) * cmax * E + el;
        double s = 0.0;
        for (int ch = 0; ch < nch; ++ch) s += g[(int64_t)ch * E];
        return s;
    };
    double b = 0.0, cu = 0.0, cv = 0.0;
    for (int el = t; el < E; el += 1024) {
        const double gu = gel(0, el), gv = gel(1, el);
        b += gu * gv;
        if (want_grad) {
            cu += gel(2, el) * gv;
            cv += gel(3, el) * gu;
        }
    }
    sh[0][t] = b; sh[1][t] = cu; sh[2][t] = cv;
    __syncthreads();
    if (t < KC) {   // the threads of one column, in thread order
        double su = 0.0, sv = 0.0;
        for (int r = 0; r < 1024 / KC; ++r) { su += sh[1][t + KC * r]; sv += sh[2][t + KC * r]; }
        col[0][t] = su; col[1][t] = sv;
    }
    for (int o = 512; o > 0; o >>= 1) {   // binary tree over the threads
        __syncthreads();
        if (t < o) sh[0][t] += sh[0][t + o];
    }
    __syncthreads();
    if (t < 64) {   // wave 0 writes the record
        double* rec = out + (int64_t)p * (2 + 2 * k);
        if (t == 0) {
            double a = 0.0;
            for (int c = 0; c < KC; ++c) a += A[c];
            rec[1] = sum_x - 2.0 * a + sh[0][0];
        }
        if (want_grad && t < k) {
            rec[2 + t] = A[KC + t] - col[0][t];
            rec[2 + k + t] = A[2 * KC + t] - col[1][t];
        }
        __threadfence_system();
        if (t == 0) {
            rec[0] = seq;   // the point's stamp, behind its values (every point's stamp is checked by a polling host: thresh_trace.hip)
            __threadfence_system();
            const unsigned done = atomicAdd(counter, 1u);
            if (done == (unsigned)npoints - 1) {
                *counter = 0u;   // ready for the next call on this stream
                __threadfence_system();
                out[(int64_t)npoints * (2 + 2 * k)] = seq;
            }
        }
    }
}

}  // namespace

extern "C" int bmf_thresh_cols64_max_points(int k) {
    if (k < 1 || k > 64) return BMF_ERR_BAD_ARG;
    const int n = BMF_COLS_MAX_GROUPS * (64 / kc_of(k));
    return n < 32 ? n : 32;
}

// doubles of workspace for up to max_points points; the first word is the completion counter of the final kernel
extern "C" int64_t bmf_thresh_cols64_work(int32_t m, int32_t n, int k, int max_points) {
    if (m < 1 || n < 1 || k < 1 || k > 64 || max_points < 1 || max_points > bmf_thresh_cols64_max_points(k)) return BMF_ERR_BAD_ARG;
    const int kc = kc_of(k), ppi = 64 / kc;
    const int64_t pa = (int64_t)((max_points + ppi - 1) / ppi) * ppi;
    const int64_t mrows = (int64_t)m + 1, nrows = (int64_t)n + 1;
    const int64_t cr = 4096 / kc;
    const int64_t uch = (mrows + cr - 1) / cr, vch = (nrows + cr - 1) / cr, cmax = uch > vch ? uch : vch;
    return 2 + BMF_COLS_STAGE + 2 * pa * (mrows + nrows) * kc + BMF_COLS_CELL_BLOCKS * pa * 3 * kc + 4 * pa * cmax * kc * kc;
}

extern "C" int bmf_thresh_cols64(const int32_t* seg_row, const int64_t* seg_beg, const int32_t* seg_len, int32_t nseg, const int32_t* idx, int32_t m,
                                 int32_t n, const double* U64, const double* V64, int64_t ldf, int k, const double* x, int32_t n_points, double lamda,
                                 double sum_x, int want_grad, double* work, double* out_host, double seq, void* stream) {
    BMF_REQUIRE(seg_row && seg_beg && seg_len && idx && U64 && V64 && x && work && out_host, "bmf_thresh_cols64: null pointer");
    BMF_REQUIRE(k >= 1 && k <= 64, "bmf_thresh_cols64: k=%d outside 1..64", k);
    BMF_REQUIRE(m >= 1 && n >= 1, "bmf_thresh_cols64: m=%d, n=%d must be >= 1", m, n);
    BMF_REQUIRE(ldf >= k, "bmf_thresh_cols64: ldf=%lld < k=%d", (long long)ldf, k);
    BMF_REQUIRE(nseg >= 1 && nseg <= BMF_COLS_MAX_SEGMENTS(m), "bmf_thresh_cols64: nseg=%d outside 1..%lld", nseg, (long long)BMF_COLS_MAX_SEGMENTS(m));
    BMF_REQUIRE(n_points >= 1 && n_points <= bmf_thresh_cols64_max_points(k), "bmf_thresh_cols64: n_points=%d outside 1..%d for k=%d", n_points,
                bmf_thresh_cols64_max_points(k), k);
    BMF_REQUIRE(bmf_aligned16(work) && bmf_aligned16(out_host), "bmf_thresh_cols64: work / out_host not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int kc = kc_of(k), ppi = 64 / kc;
    const int G = (n_points + ppi - 1) / ppi, pa = G * ppi;
    const int64_t mrows = (int64_t)m + 1, nrows = (int64_t)n + 1;
    BMF_REQUIRE(mrows * kc < (1ll << 31) && nrows * kc < (1ll << 31), "bmf_thresh_cols64: factor too large");
    const int cr = 4096 / kc;
    const int uch = (int)((mrows + cr - 1) / cr), vch = (int)((nrows + cr - 1) / cr), cmax = uch > vch ? uch : vch;
    const int nbmax = BMF_COLS_CELL_BLOCKS;
    const int nb = (nseg + 3) / 4 < nbmax ? (nseg + 3) / 4 : nbmax;   // a function of nseg alone: the same sums on every call
    unsigned* counter = reinterpret_cast<unsigned*>(work);
    double* xs = work + 2;
    double* Us = xs + BMF_COLS_STAGE;
    double* dUs = Us + (int64_t)pa * mrows * kc;
    double* Vs = dUs + (int64_t)pa * mrows * kc;
    double* dVs = Vs + (int64_t)pa * nrows * kc;
    double* cellpart = dVs + (int64_t)pa * nrows * kc;
    double* grampart = cellpart + (int64_t)nbmax * pa * 3 * kc;
    const int kshift = kc == 16 ? 4 : (kc == 32 ? 5 : 6);
    int gu = (int)((mrows * kc + 255) / 256), gv = (int)((nrows * kc + 255) / 256);
    if (gu > 1024) gu = 1024;
    if (gv > 1024) gv = 1024;
    BMF_LAUNCH(cols_stage_kernel, dim3(1), dim3(1024), 0, s, x, n_points, k, kc, pa, xs);
    BMF_LAUNCH(cols_transform_kernel, dim3((unsigned)(gu + gv), (unsigned)pa), dim3(256), 0, s, U64, ldf, m, mrows, V64, n, nrows, k, kshift, lamda, xs, Us,
               want_grad ? dUs : nullptr, Vs, want_grad ? dVs : nullptr, gu);
    const int gram_blocks = pa * (want_grad ? 2 : 1) * (uch + vch);
    // the cell pass runs in slices of two groups of points whose transformed V stays resident in an XCD's L2 (thresh_trace.hip)
    constexpr int gp = 2;
#define BMF_COLS_CELLS(KC_, GR_, GM_)                                                                                                        \
    BMF_LAUNCH((cols_cells_kernel<KC_, GR_, GM_>), dim3((unsigned)nb), dim3(256), 0, s, seg_row, seg_beg, seg_len, idx, nseg, mrows, nrows, gq, \
               Us + (int64_t)g0 * ppi * mrows * KC_, dUs + (int64_t)g0 * ppi * mrows * KC_, Vs + (int64_t)g0 * ppi * nrows * KC_,              \
               dVs + (int64_t)g0 * ppi * nrows * KC_, cellpart + (int64_t)g0 * ppi * nbmax * 3 * KC_, nbmax)
#define BMF_COLS_MAIN(KC_)                                                                                                                   \
    if (kc == KC_) {                                                                                                                         \
        if (want_grad) BMF_LAUNCH((trace_gram_kernel<KC_, true>), dim3((unsigned)gram_blocks), dim3(256), 0, s, mrows, nrows, pa, Us, dUs, Vs, dVs, grampart, uch, vch); \
        else BMF_LAUNCH((trace_gram_kernel<KC_, false>), dim3((unsigned)gram_blocks), dim3(256), 0, s, mrows, nrows, pa, Us, dUs, Vs, dVs, grampart, uch, vch); \
        for (int g0 = 0; g0 < G; g0 += gp) {                                                                                                 \
            const int gq = G - g0 < gp ? G - g0 : gp;                                                                                        \
            if (want_grad) {                                                                                                                 \
                if (gq == 1) BMF_COLS_CELLS(KC_, true, 1); else BMF_COLS_CELLS(KC_, true, 2);                                                \
            } else {                                                                                                                         \
                if (gq == 1) BMF_COLS_CELLS(KC_, false, 1); else BMF_COLS_CELLS(KC_, false, 2);                                              \
            }                                                                                                                                \
        }                                                                                                                                    \
        BMF_LAUNCH((cols_final_kernel<KC_>), dim3((unsigned)n_points), dim3(1024), 0, s, cellpart, grampart, nb, nbmax, n_points, pa, uch, vch, k, sum_x, \
                   want_grad, out_host, seq, counter);                                                                                       \
    }
    BMF_COLS_MAIN(16) BMF_COLS_MAIN(32) BMF_COLS_MAIN(64)
#undef BMF_COLS_CELLS
#undef BMF_COLS_MAIN
    (void)cmax;
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}
