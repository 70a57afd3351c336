// The objective of FastStep for one factor, fp64 end to end (PyBMF/models/FastStep.py:147-211).
//
//   M = 2 X - 1,  S = U V^T with column k replaced by the candidate (u, v),  a = -M o (S - tau)
//   F  = sum over all cells of log(1 + exp(W o a))                                                        :147-172
//   G  = W o (-M o sigmoid(a)),  du = G v,  dv = G^T u                                                    :175-211
//   X_pd = S > tau -> TP, FP against X                                                                    :105, utils/common.py:64-79
//
// Only column k moves while factor k is searched, so S - tau = B + u v^T with B = U V^T - U[:, k] V[:, k]^T - tau built once per
// (round, k) (faststep_base_kernel) and one streaming pass over B and the bits of X per evaluation (faststep_eval_kernel): 8 bytes of
// B + 1 / 8 byte of X (+ 1 / 8 of the mask) per cell, one exp, one log1p and -- with the gradient -- one division per cell.  The
// line search compares F values that differ by min_diff = 1e-2 on F of 1e3 .. 1e7 (as in csrc/thresh64.hip): B, the per-cell
// arithmetic and every sum are fp64.  Row sums (du) and column sums (dv) leave the pass as one partial slab per tile column / tile
// row; faststep_reduce_kernel adds the slabs, the per-tile F and the per-tile counts in a fixed order.  No atomics anywhere: the
// same input gives the same bits.
#include "common.h"

namespace {

constexpr int TR = 64;    // rows of a tile: 4 waves x 16 rows
constexpr int TC = 128;   // columns of a tile: 64 lanes x 2 columns (one 16-byte load of B per lane and row)

// B = U V^T - tau without latent column `skip`.  One block = a 64 x 64 tile, thread (ty, tx) = rows 4 ty .. 4 ty + 3, columns
// 4 tx .. 4 tx + 3; the factor tiles go through LDS 16 latent columns at a time, transposed (as dense64_kernel, thresh64.hip).
// Runs once per (round, k) against hundreds of evaluations: plain fp64 FMAs.
__global__ __launch_bounds__(256) void faststep_base_kernel(const double* __restrict__ U, const double* __restrict__ V, int kp, int k,
                                                             int skip, double tau, double* __restrict__ B, int64_t ldb) {
    __shared__ double a_t[16][64], b_t[16][64];
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    const int64_t i0 = (int64_t)blockIdx.y * 64, j0 = (int64_t)blockIdx.x * 64;
    double p[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) p[a][b] = 0.0;
    for (int k0 = 0; k0 < k; k0 += 16) {
        __syncthreads();
        for (int e = t; e < 64 * 16; e += 256) {
            const int kk = e >> 6, row = e & 63;
            const bool on = k0 + kk < k && k0 + kk != skip;
            a_t[kk][row] = on ? U[(i0 + row) * kp + k0 + kk] : 0.0;
            b_t[kk][row] = on ? V[(j0 + row) * kp + k0 + kk] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < 16; ++kk) {
            double a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = a_t[kk][4 * ty + q];
                b[q] = b_t[kk][4 * tx + q];
            }
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) p[x][y] = fma(a[x], b[y], p[x][y]);
        }
    }
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        double* dst = B + (i0 + 4 * ty + x) * ldb + j0 + 4 * tx;
        *reinterpret_cast<double2*>(dst) = make_double2(p[x][0] - tau, p[x][1] - tau);
        *reinterpret_cast<double2*>(dst + 2) = make_double2(p[x][2] - tau, p[x][3] - tau);
    }
}

// One cell.  s = S - tau; a = -M s; softplus(a) = max(a, 0) + log1p(exp(-|a|)) and the piecewise sigmoid of utils/common.py:82-89
// (1 / (1 + exp(-a)) for a >= 0, exp(a) / (1 + exp(a)) below) share the one exp(-|a|).  A cell the mask leaves out adds log 2 to F
// and nothing to the gradient; the counts take every cell.
template <bool GRAD, bool MASK>
__device__ __forceinline__ void faststep_cell(double b, bool x, bool w, bool in, double ui, double vj, bool count, double& f, double& rs,
                                              double& cs, unsigned& tp, unsigned& fp) {
    const double s = fma(ui, vj, b);
    if (count) {
        const bool pd = in && s > 0.0;
        tp += (pd && x) ? 1u : 0u;
        fp += (pd && !x) ? 1u : 0u;
    }
    const double a = x ? -s : s;
    const double e = exp(-fabs(a));
    double sp = fmax(a, 0.0) + log1p(e);
    double g = 0.0;
    if (GRAD) {
        const double sig = (a >= 0.0 ? 1.0 : e) / (1.0 + e);
        g = x ? -sig : sig;
    }
    if (MASK && !w) {
        sp = 0.6931471805599453;   // log(1 + exp(0))
        g = 0.0;
    }
    f += in ? sp : 0.0;
    if (GRAD) {
        g = in ? g : 0.0;
        rs = fma(g, vj, rs);
        cs = fma(g, ui, cs);
    }
}

// Block (bx, by) = rows [64 by, 64 by + 64) x columns [128 bx, 128 bx + 128); wave w takes rows 16 w .. 16 w + 15, lane l columns
// 2 l, 2 l + 1.  Out: du_part[bx][row] (the tile's share of the row sums: per-lane shares staged in LDS, added in lane order),
// dv_part[by][column] (the four waves' shares added in wave order), f_part / c_part[by * gridDim.x + bx].
template <bool GRAD, bool MASK>
__global__ __launch_bounds__(256) void faststep_eval_kernel(const double* __restrict__ B, int64_t ldb, const uint32_t* __restrict__ Xbits,
                                                             const uint32_t* __restrict__ Wbits, int64_t ldx, int m, int n,
                                                             const double* __restrict__ u, const double* __restrict__ v, int want_counts,
                                                             double* __restrict__ du_part, int64_t m_pad, double* __restrict__ dv_part,
                                                             int64_t n_pad, double* __restrict__ f_part, uint32_t* __restrict__ c_part) {
    __shared__ double rowred[GRAD ? TR : 1][65];
    __shared__ double colred[GRAD ? 4 : 1][TC];
    __shared__ double fred[4];
    __shared__ unsigned cred[4][2];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t i0 = (int64_t)blockIdx.y * TR + wave * 16, j = (int64_t)blockIdx.x * TC + 2 * lane;
    const bool in0 = j < n, in1 = j + 1 < n;
    const double v0 = in0 ? v[j] : 0.0, v1 = in1 ? v[j + 1] : 0.0;
    const int64_t word = j >> 5;
    const int sh = (int)(j & 31);
    const bool count = want_counts != 0;
    double f = 0.0, dv0 = 0.0, dv1 = 0.0;
    unsigned tp = 0, fp = 0;
    const int rows = (int)min((int64_t)16, max((int64_t)0, (int64_t)m - i0));   // wave-uniform
    for (int r = 0; r < rows; ++r) {
        const int64_t i = i0 + r;
        const double2 b = *reinterpret_cast<const double2*>(B + i * ldb + j);
        const unsigned xw = Xbits[i * ldx + word] >> sh;
        const unsigned ww = MASK ? Wbits[i * ldx + word] >> sh : 3u;
        const double ui = u[i];
        double rs = 0.0;
        faststep_cell<GRAD, MASK>(b.x, (xw & 1u) != 0, (ww & 1u) != 0, in0, ui, v0, count, f, rs, dv0, tp, fp);
        faststep_cell<GRAD, MASK>(b.y, (xw & 2u) != 0, (ww & 2u) != 0, in1, ui, v1, count, f, rs, dv1, tp, fp);
        if (GRAD) rowred[wave * 16 + r][lane] = rs;
    }
    if (GRAD) {
        for (int r = rows; r < 16; ++r) rowred[wave * 16 + r][lane] = 0.0;
        colred[wave][2 * lane] = dv0;
        colred[wave][2 * lane + 1] = dv1;
    }
    f = wave_sum(f);
    tp = wave_sum(tp);
    fp = wave_sum(fp);
    if (lane == 0) { fred[wave] = f; cred[wave][0] = tp; cred[wave][1] = fp; }
    __syncthreads();
    if (GRAD) {
        // row sums: four threads per row, each adds 16 lanes' shares in lane order, then the four quarter sums pairwise
        const int row = t >> 2, part = t & 3;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) s += rowred[row][part * 16 + q];
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        if (part == 0) du_part[(int64_t)blockIdx.x * m_pad + (int64_t)blockIdx.y * TR + row] = s;
        if (t < TC)
            dv_part[(int64_t)blockIdx.y * n_pad + (int64_t)blockIdx.x * TC + t] = ((colred[0][t] + colred[1][t]) + colred[2][t]) + colred[3][t];
    }
    if (t == 0) {
        const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        f_part[blk] = ((fred[0] + fred[1]) + fred[2]) + fred[3];
        c_part[2 * blk] = cred[0][0] + cred[1][0] + cred[2][0] + cred[3][0];
        c_part[2 * blk + 1] = cred[0][1] + cred[1][1] + cred[2][1] + cred[3][1];
    }
}

// Blocks [0, gu): du[i] = sum over the ntc tile columns of du_part, in order; blocks [gu, gu + gv): dv[j] likewise over the ntr tile
// rows; the last block: F and the counts over the nblk tiles (thread t adds tiles t, t + 256, ... in order, then a tree).
__global__ __launch_bounds__(256) void faststep_reduce_kernel(const double* __restrict__ du_part, int64_t m_pad, int ntc, int m,
                                                               double* __restrict__ du, int gu, const double* __restrict__ dv_part,
                                                               int64_t n_pad, int ntr, int n, double* __restrict__ dv, int gv,
                                                               const double* __restrict__ f_part, const uint32_t* __restrict__ c_part,
                                                               int64_t nblk, double* __restrict__ F, int64_t* __restrict__ counts) {
    const int t = threadIdx.x;
    int b = blockIdx.x;
    if (b < gu) {
        const int64_t i = (int64_t)b * 256 + t;
        if (i < m) {
            double s = 0.0;
            for (int c = 0; c < ntc; ++c) s += du_part[(int64_t)c * m_pad + i];
            du[i] = s;
        }
        return;
    }
    b -= gu;
    if (b < gv) {
        const int64_t j = (int64_t)b * 256 + t;
        if (j < n) {
            double s = 0.0;
            for (int r = 0; r < ntr; ++r) s += dv_part[(int64_t)r * n_pad + j];
            dv[j] = s;
        }
        return;
    }
    __shared__ double red[256];
    __shared__ unsigned long long cred[2][256];
    double s = 0.0;
    unsigned long long tp = 0, fp = 0;
    for (int64_t q = t; q < nblk; q += 256) {
        s += f_part[q];
        tp += c_part[2 * q];
        fp += c_part[2 * q + 1];
    }
    red[t] = s;
    cred[0][t] = tp;
    cred[1][t] = fp;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            red[t] += red[t + o];
            cred[0][t] += cred[0][t + o];
            cred[1][t] += cred[1][t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        F[0] = red[0];
        if (counts) {
            counts[0] = (int64_t)cred[0][0];
            counts[1] = (int64_t)cred[1][0];
        }
    }
}

}  // namespace

extern "C" int bmf_faststep_base(const double* U64, const double* V64, int64_t m_pad, int64_t n_pad, int32_t m, int32_t n, int k, int kp,
                                 int skip, double tau, double* B, void* stream) {
    BMF_REQUIRE(U64 && V64 && B, "bmf_faststep_base: null pointer");
    BMF_REQUIRE(m >= 1 && n >= 1 && m <= m_pad && n <= n_pad && m_pad % 128 == 0 && n_pad % 128 == 0, "bmf_faststep_base: bad shape");
    BMF_REQUIRE((kp == 32 || kp == 64) && k >= 1 && k <= kp && skip >= -1 && skip < k, "bmf_faststep_base: need 1 <= k <= kp, kp in {32,64}, -1 <= skip < k");
    // the tiles the evaluation reads: whole 128-column tiles over n, 64-row tiles over m (inside the padding: m_pad, n_pad % 128 == 0)
    dim3 grid((unsigned)(((int64_t)n + TC - 1) / TC * 2), (unsigned)(((int64_t)m + 63) / 64)), block(256);
    BMF_LAUNCH(faststep_base_kernel, grid, block, 0, (hipStream_t)stream, U64, V64, kp, k, skip, tau, B, n_pad);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int64_t bmf_faststep_eval_work(int64_t m_pad, int64_t n_pad, int32_t m, int32_t n) {
    if (m < 1 || n < 1 || m > m_pad || n > n_pad || m_pad % 128 || n_pad % 128) return BMF_ERR_BAD_ARG;
    const int64_t ntr = ((int64_t)m + TR - 1) / TR, ntc = ((int64_t)n + TC - 1) / TC;
    return ntc * m_pad + ntr * n_pad + 2 * ntr * ntc;   // du slabs | dv slabs | F per tile | (TP, FP) per tile as two uint32
}

extern "C" int bmf_faststep_eval(const double* B, const uint32_t* Xbits, const uint32_t* Wbits, int64_t m_pad, int64_t n_pad, int64_t ldx,
                                 int32_t m, int32_t n, const double* u, const double* v, int want_grad, int want_counts, double* work,
                                 double* F, double* du, double* dv, int64_t* counts, void* stream) {
    BMF_REQUIRE(B && Xbits && u && v && work && F, "bmf_faststep_eval: null pointer");
    BMF_REQUIRE(m >= 1 && n >= 1 && m <= m_pad && n <= n_pad && m_pad % 128 == 0 && n_pad % 128 == 0, "bmf_faststep_eval: bad shape");
    BMF_REQUIRE(ldx * 32 >= n_pad, "bmf_faststep_eval: ldx does not cover n_pad");
    BMF_REQUIRE(!want_grad || (du && dv), "bmf_faststep_eval: want_grad needs du and dv");
    BMF_REQUIRE(!want_counts || counts, "bmf_faststep_eval: want_counts needs counts");
    BMF_REQUIRE(bmf_aligned16(B), "bmf_faststep_eval: B must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int64_t ntr = ((int64_t)m + TR - 1) / TR, ntc = ((int64_t)n + TC - 1) / TC;
    BMF_REQUIRE(ntr <= 65535, "bmf_faststep_eval: more than 65535 row tiles");
    double* du_part = work;
    double* dv_part = du_part + ntc * m_pad;
    double* f_part = dv_part + ntr * n_pad;
    uint32_t* c_part = reinterpret_cast<uint32_t*>(f_part + ntr * ntc);
    dim3 grid((unsigned)ntc, (unsigned)ntr), block(256);
#define BMF_FS_EVAL(GR_, MK_)                                                                                                          \
    BMF_LAUNCH((faststep_eval_kernel<GR_, MK_>), grid, block, 0, s, B, n_pad, Xbits, Wbits, ldx, m, n, u, v, want_counts, du_part, m_pad, \
               dv_part, n_pad, f_part, c_part)
    if (want_grad) { if (Wbits) BMF_FS_EVAL(true, true); else BMF_FS_EVAL(true, false); }
    else { if (Wbits) BMF_FS_EVAL(false, true); else BMF_FS_EVAL(false, false); }
#undef BMF_FS_EVAL
    const int gu = want_grad ? (m + 255) / 256 : 0, gv = want_grad ? (n + 255) / 256 : 0;
    BMF_LAUNCH(faststep_reduce_kernel, dim3((unsigned)(gu + gv + 1)), dim3(256), 0, s, du_part, m_pad, (int)ntc, m, du, gu, dv_part, n_pad,
               (int)ntr, n, dv, gv, f_part, c_part, ntr * ntc, F, want_counts ? counts : nullptr);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}
