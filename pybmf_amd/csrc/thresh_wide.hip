// The thresholding objective of BinaryMFThreshold at a rank 64 < k <= 128 (PyBMF/models/BinaryMFThreshold.py:150-207), fp64 throughout:
// the trace form for the all-ones mask (the mathematics is the header of thresh_trace.hip) and the pass over a list of observed cells
// (thresh64.hip), both on transformed factors of 128 columns.
//
// Layout.  A transformed factor is rows x 128 doubles, row after row; columns >= k and padding rows are exact zero, so no kernel behind
// the transform looks at k again.  A LANE HOLDS TWO ADJACENT COLUMNS (2 l, 2 l + 1) of one pair: a row of a factor is one 16-byte load
// per lane and 1 KiB per wave, and a cell's dot product is two FMAs per lane and one sum over the 64 lanes.
//
// Trace form, per call of up to 8 (u, v) pairs:
//   transform   S[p][row][128] (and D) for every pair; one extra all-zero row that the cell pass points missing cells at
//   Gram        Us^T Us, Vs^T Vs (and Us^T dUs, Vs^T dVs) as 128 x 128 matrices, cross terms between the two 64-column halves included.
//               A workgroup keeps an 8 x 8 register tile per thread over ALL its rows (16 rows at a time through the LDS); the rows of a
//               factor are cut into at most 32 chunks (of at least 256 rows), so a factor costs at most 32 partial Grams of 128 KiB per
//               matrix and pair, whatever its length -- 4 MiB instead of the 400 MB that 4096 / 128 rows per partial would take at 100 000
//               rows.  The chunking depends on the shape alone, never on the device.
//   cells       one wave per segment of the ones (<= 128 cells of one row), two pairs per pass: the transformed V of one pair is 3.8 MB
//               at MovieLens-1M shape against 4 MiB of L2 per XCD, the byte count at which thresh_trace.hip measured two groups per
//               pass as the best slice (the slice width itself was not measured again here)
//   final       one workgroup per pair: the ordered sums, F and dF, and the stamps of bmf_thresh_trace64's output protocol
// Every partial is written to its own slot and added in a fixed order; no floating-point atomics: the same input gives the same bits.
#include "common.h"

#define BMF_TW_KC 128                                        // columns of a transformed factor
#define BMF_TW_MAX_PAIRS 8
#define BMF_TW_MAX_SEGMENTS(m) ((int64_t)8 * (m) + 64)       // as bmf_thresh_trace64
#define BMF_TW_MAX_CHUNKS 32                                 // partial Grams per factor, matrix and pair
#define BMF_TW_CHUNK_ROWS 256                                // least rows of a chunk (a multiple of BMF_TW_TILE_ROWS)
#define BMF_TW_TILE_ROWS 16                                  // rows that pass through the LDS at a time

namespace {

typedef __attribute__((ext_vector_type(2))) double f64x2;

struct WidePairs {
    double u[BMF_TW_MAX_PAIRS], v[BMF_TW_MAX_PAIRS];
};

// the transform of the trace form at k <= 64 (thresh_trace.hip)
__device__ __forceinline__ void sigmoid_pair_tw(double z, double lam, double& s, double& d) {
    if (z >= 0) s = 1.0 / (1.0 + exp(-z));
    else { const double e = exp(z); s = e / (1.0 + e); }
    d = lam * s * (1.0 - s);
}
// the transform of the cell-list form at k <= 64 (thresh64.hip): d = lam exp(-z) s^2 without overflow or cancellation
__device__ __forceinline__ void sigmoid_pair_mw(double z, double lam, double& s, double& d) {
    const double e = exp(-fabs(z));
    if (z >= 0) { s = 1.0 / (1.0 + e); d = lam * e * s * s; }
    else { s = e / (1.0 + e); d = lam * s / (1.0 + e); }
}

// rows of a Gram chunk for a factor of `rows` rows: at least BMF_TW_CHUNK_ROWS, a multiple of BMF_TW_TILE_ROWS, at most
// BMF_TW_MAX_CHUNKS chunks (host and device)
__host__ __device__ inline int64_t tw_chunk_rows(int64_t rows) {
    int64_t cr = (rows + BMF_TW_MAX_CHUNKS - 1) / BMF_TW_MAX_CHUNKS;
    cr = (cr + BMF_TW_TILE_ROWS - 1) / BMF_TW_TILE_ROWS * BMF_TW_TILE_ROWS;
    return cr < BMF_TW_CHUNK_ROWS ? BMF_TW_CHUNK_ROWS : cr;
}
__host__ __device__ inline int tw_chunks(int64_t rows) { return (int)((rows + tw_chunk_rows(rows) - 1) / tw_chunk_rows(rows)); }

// S[p][row][c], c < 128, of pair p = blockIdx.y (zero for rows >= m / n and columns >= k; row `mrows - 1` / `nrows - 1` is the zero row of
// the cell pass).  Blocks [0, gu) of a pair do U, the rest V.
__global__ __launch_bounds__(256) void tw_transform_kernel(const double* __restrict__ U, int64_t ldf, int m, int64_t mrows, const double* __restrict__ V,
                                                            int n, int64_t nrows, int k, double lam, WidePairs pr, double* __restrict__ Us,
                                                            double* __restrict__ dUs, double* __restrict__ Vs, double* __restrict__ dVs, int gu) {
    const bool is_u = (int)blockIdx.x < gu;
    const int p = (int)blockIdx.y;
    const double* F = is_u ? U : V;
    const int rows = is_u ? m : n;
    const int per_pair = (int)((is_u ? mrows : nrows) * BMF_TW_KC);   // < 2^31: checked by the launcher
    double* S = (is_u ? Us : Vs) + (int64_t)p * per_pair;
    double* D = (is_u ? dUs : dVs);
    if (D) D += (int64_t)p * per_pair;
    const double x = is_u ? pr.u[p] : pr.v[p];
    const int b = is_u ? (int)blockIdx.x : (int)blockIdx.x - gu, nb = is_u ? gu : (int)gridDim.x - gu;
    for (int64_t i = (int64_t)b * 256 + threadIdx.x; i < per_pair; i += (int64_t)nb * 256) {
        const int r = (int)(i / BMF_TW_KC), c = (int)(i % BMF_TW_KC);
        double s_ = 0.0, d_ = 0.0;
        if (r < rows && c < k) sigmoid_pair_tw((F[(int64_t)r * ldf + c] - x) * lam, lam, s_, d_);   // (padding is never read: it may hold anything)
        S[i] = s_;
        if (D) D[i] = d_;
    }
}

// A wave takes one segment of the ones; lane l serves columns 2 l, 2 l + 1 of pairs g < G <= GMAX.  Per cell (i, j) and pair one 16-byte
// load of Vs (one of dVs) and two (six) FMAs.  The wave fetches 64 column indices with one load and walks them T at a time (v_readlane:
// the indices are wave-uniform; missing cells point at the zero row and add exact zeros), so T * G independent loads are in flight per
// lane.  cellpart[p][kind][segment] = sum over the segment's ones of <Us_i, Vs_j>, <dUs_i, Vs_j>, <Us_i, dVs_j>.  The sum <Us_i, Vs_j> is
// formed by the same instructions in the same order with and without the gradient.
template <bool GRAD, int GMAX>
__global__ __launch_bounds__(256) void tw_cells_kernel(const int32_t* __restrict__ seg_row, const int64_t* __restrict__ seg_beg,
                                                        const int32_t* __restrict__ seg_len, const int32_t* __restrict__ idx, int nseg, int64_t mrows,
                                                        int64_t nrows, int G, const double* __restrict__ Us, const double* __restrict__ dUs,
                                                        const double* __restrict__ Vs, const double* __restrict__ dVs, double* __restrict__ cellpart) {
    constexpr int T = (GRAD ? 8 : 16) / GMAX;   // cells per trip (divides 64)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sg = (int)blockIdx.x * 4 + wave;
    if (sg >= nseg) return;
    const int i = seg_row[sg];
    const int64_t w0 = seg_beg[sg];
    const int len = seg_len[sg];   // <= 128
    const int64_t upair = mrows * BMF_TW_KC, vpair = nrows * BMF_TW_KC;
    f64x2 us[GMAX], dus[GMAX];
    double a0[GMAX], a1[GMAX], a2[GMAX];
#pragma unroll
    for (int g = 0; g < GMAX; ++g) {
        const f64x2 zero = {0.0, 0.0};
        us[g] = g < G ? *reinterpret_cast<const f64x2*>(Us + g * upair + (int64_t)i * BMF_TW_KC + 2 * lane) : zero;
        dus[g] = (GRAD && g < G) ? *reinterpret_cast<const f64x2*>(dUs + g * upair + (int64_t)i * BMF_TW_KC + 2 * lane) : zero;
        a0[g] = a1[g] = a2[g] = 0.0;
    }
    const int zrow = (int)(nrows - 1);   // all-zero row
    const double* vlane = Vs + 2 * lane;
    const double* dlane = dVs + 2 * lane;
    const int myj0 = lane < len ? idx[w0 + lane] : zrow;
    const int myj1 = 64 + lane < len ? idx[w0 + 64 + lane] : zrow;
    for (int st = 0; st < len; st += 64) {
        const int myj = st == 0 ? myj0 : myj1;
        const int nst = min(64, len - st);
        for (int t0 = 0; t0 < nst; t0 += T) {
            f64x2 vv[T][GMAX], dv[T][GMAX];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int64_t jo = (int64_t)__builtin_amdgcn_readlane(myj, t0 + t) * BMF_TW_KC;   // (t0 + t < 64: T divides 64)
#pragma unroll
                for (int g = 0; g < GMAX; ++g)
                    if (g < G) {
                        vv[t][g] = *reinterpret_cast<const f64x2*>(vlane + g * vpair + jo);
                        if (GRAD) dv[t][g] = *reinterpret_cast<const f64x2*>(dlane + g * vpair + jo);
                    }
            }
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int g = 0; g < GMAX; ++g)
                    if (g < G) {
                        a0[g] = fma(us[g].x, vv[t][g].x, a0[g]);
                        a0[g] = fma(us[g].y, vv[t][g].y, a0[g]);
                        if (GRAD) {
                            a1[g] = fma(dus[g].x, vv[t][g].x, a1[g]);
                            a1[g] = fma(dus[g].y, vv[t][g].y, a1[g]);
                            a2[g] = fma(us[g].x, dv[t][g].x, a2[g]);
                            a2[g] = fma(us[g].y, dv[t][g].y, a2[g]);
                        }
                    }
        }
    }
    // the 64 lanes of a pair are summed in a fixed order (butterfly), lane 0 writes
#pragma unroll
    for (int g = 0; g < GMAX; ++g)
        if (g < G) {
            const double s0 = wave_sum(a0[g]);
            if (lane == 0) cellpart[((int64_t)g * 3 + 0) * nseg + sg] = s0;
            if (GRAD) {
                const double s1 = wave_sum(a1[g]), s2 = wave_sum(a2[g]);
                if (lane == 0) { cellpart[((int64_t)g * 3 + 1) * nseg + sg] = s1; cellpart[((int64_t)g * 3 + 2) * nseg + sg] = s2; }
            }
        }
}

// One partial Gram S^T D (128 x 128) over one chunk of rows of one factor of one pair; D = S for the first two matrices.  Thread
// (ty, tx) of 16 x 16 holds the 8 x 8 elements (ca, cb), ca = 32 (a >> 1) + 2 ty + (a & 1), cb = 32 (b >> 1) + 2 tx + (b & 1): its eight
// values of a row are four 16-byte LDS reads at a stride of 256 bytes, and the 16 tx of a wave read 256 contiguous bytes with each of
// them (no bank conflict; the four ty of a wave are broadcasts).  The accumulators stay in registers over the whole chunk.
// grampart[q][p][chunk][128 * 128], q = 0: Us^T Us, 1: Vs^T Vs, 2: Us^T dUs, 3: Vs^T dVs; chunk slots: max(uchunks, vchunks).
__global__ __launch_bounds__(256) void tw_gram_kernel(int64_t mrows, int64_t nrows, int npairs, int want_grad, const double* __restrict__ Us,
                                                       const double* __restrict__ dUs, const double* __restrict__ Vs, const double* __restrict__ dVs,
                                                       double* __restrict__ grampart, int uchunks, int vchunks) {
    __shared__ __attribute__((aligned(16))) double sS[BMF_TW_TILE_ROWS * BMF_TW_KC], sD[BMF_TW_TILE_ROWS * BMF_TW_KC];   // 16 KiB each
    const int per_pair_blocks = (want_grad ? 2 : 1) * (uchunks + vchunks);
    const int p = (int)blockIdx.x / per_pair_blocks;
    int r = (int)blockIdx.x % per_pair_blocks;
    const bool second = r >= uchunks + vchunks;   // the S^T D matrices
    if (second) r -= uchunks + vchunks;
    const bool is_u = r < uchunks;
    const int chunk = is_u ? r : r - uchunks;
    const int64_t ralloc = is_u ? mrows : nrows;
    const double* S = (is_u ? Us : Vs) + (int64_t)p * ralloc * BMF_TW_KC;
    const double* D = second ? ((is_u ? dUs : dVs) + (int64_t)p * ralloc * BMF_TW_KC) : S;
    const int64_t cr = tw_chunk_rows(ralloc);
    const int64_t r0 = (int64_t)chunk * cr, r1 = min(ralloc, r0 + cr);
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    double acc[8][8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = 0.0;
    for (int64_t rt = r0; rt < r1; rt += BMF_TW_TILE_ROWS) {
        const int64_t left = (r1 - rt) * (BMF_TW_KC / 2);   // 16-byte units of this tile that exist
        __syncthreads();
#pragma unroll
        for (int e = 0; e < BMF_TW_TILE_ROWS * BMF_TW_KC / 2 / 256; ++e) {
            const int q = t + 256 * e;
            const f64x2 zero = {0.0, 0.0};
            const bool in = q < left;
            reinterpret_cast<f64x2*>(sS)[q] = in ? reinterpret_cast<const f64x2*>(S + rt * BMF_TW_KC)[q] : zero;
            reinterpret_cast<f64x2*>(sD)[q] = in ? reinterpret_cast<const f64x2*>(D + rt * BMF_TW_KC)[q] : zero;
        }
        __syncthreads();
#pragma unroll 2
        for (int row = 0; row < BMF_TW_TILE_ROWS; ++row) {   // (rows past the chunk's end are zeros: they add nothing)
            double sv[8], dv[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f64x2 s2 = *reinterpret_cast<const f64x2*>(&sS[row * BMF_TW_KC + 32 * j + 2 * ty]);
                const f64x2 d2 = *reinterpret_cast<const f64x2*>(&sD[row * BMF_TW_KC + 32 * j + 2 * tx]);
                sv[2 * j] = s2.x; sv[2 * j + 1] = s2.y;
                dv[2 * j] = d2.x; dv[2 * j + 1] = d2.y;
            }
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int b = 0; b < 8; ++b) acc[a][b] = fma(sv[a], dv[b], acc[a][b]);
        }
    }
    const int qm = (second ? 2 : 0) + (is_u ? 0 : 1);
    const int cmax = uchunks > vchunks ? uchunks : vchunks;
    double* out = grampart + (((int64_t)qm * npairs + p) * cmax + chunk) * (BMF_TW_KC * BMF_TW_KC);
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; b += 2) {
            const int ca = 32 * (a >> 1) + 2 * ty + (a & 1), cb = 32 * (b >> 1) + 2 * tx;
            const f64x2 o = {acc[a][b], acc[a][b + 1]};
            *reinterpret_cast<f64x2*>(&out[ca * BMF_TW_KC + cb]) = o;
        }
}

// One block of 1024 threads per pair: the ordered sums, F and dF, and the output protocol of bmf_thresh_trace64 -- out[4 p + 0..3] =
// (seq, 2 F, dF_u, dF_v) in pinned host memory, the stamp behind the three results, and the LAST block to finish (a device counter)
// writes out[4 npairs] = seq; every write behind a system-scope fence.  Every sum has a fixed shape: thread-strided partial sums (an
// element's chunks in order), then a binary tree over the threads.  2 F does not depend on want_grad.
__global__ __launch_bounds__(1024) void tw_final_kernel(const double* __restrict__ cellpart, const double* __restrict__ grampart, int nseg, int npairs,
                                                         int uchunks, int vchunks, double sum_x, int want_grad, double* __restrict__ out, double seq,
                                                         unsigned* __restrict__ counter) {
    __shared__ double sh[3][1024];
    const int p = (int)blockIdx.x, t = threadIdx.x;
    auto tree = [&]() {
        __syncthreads();
        for (int o = 512; o > 0; o >>= 1) {
            if (t < o) { sh[0][t] += sh[0][t + o]; sh[1][t] += sh[1][t + o]; sh[2][t] += sh[2][t + o]; }
            __syncthreads();
        }
    };
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const double* cp = cellpart + (int64_t)p * 3 * nseg;   // [p][kind][segment]
    for (int i = t; i < nseg; i += 1024) {
        s0 += cp[i];
        if (want_grad) { s1 += cp[(int64_t)nseg + i]; s2 += cp[2 * (int64_t)nseg + i]; }
    }
    sh[0][t] = s0; sh[1][t] = s1; sh[2][t] = s2;
    tree();
    const double a = sh[0][0], du1 = sh[1][0], dv1 = sh[2][0];
    __syncthreads();
    // < GU, GV >, < GV, HU >, < GU, HV >
    const int cmax = uchunks > vchunks ? uchunks : vchunks;
    auto gel = [&](int q, int el) {
        const int nch = (q & 1) ? vchunks : uchunks;
        const double* g = grampart + ((int64_t)q * npairs + p) * cmax * (BMF_TW_KC * BMF_TW_KC) + el;
        double s = 0.0;
        for (int ch = 0; ch < nch; ++ch) s += g[(int64_t)ch * (BMF_TW_KC * BMF_TW_KC)];
        return s;
    };
    double b = 0.0, bu = 0.0, bv = 0.0;
    for (int el = t; el < BMF_TW_KC * BMF_TW_KC; el += 1024) {
        const double gu = gel(0, el), gv = gel(1, el);
        b = fma(gu, gv, b);
        if (want_grad) {
            bu = fma(gv, gel(2, el), bu);
            bv = fma(gu, gel(3, el), bv);
        }
    }
    sh[0][t] = b; sh[1][t] = bu; sh[2][t] = bv;
    tree();
    if (t == 0) {
        out[4 * p + 1] = sum_x - 2.0 * a + sh[0][0];
        out[4 * p + 2] = want_grad ? du1 - sh[1][0] : 0.0;
        out[4 * p + 3] = want_grad ? dv1 - sh[2][0] : 0.0;
        __threadfence_system();
        out[4 * p + 0] = seq;   // the pair's stamp, behind its three results (the host checks every pair's stamp: thresh_trace.hip)
        __threadfence_system();
        const unsigned done = atomicAdd(counter, 1u);
        if (done == (unsigned)npairs - 1) {
            *counter = 0u;   // ready for the next call on this stream
            __threadfence_system();
            out[4 * npairs] = seq;
        }
    }
}

// ---- the pass over a list of observed cells ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mw_transform_kernel(const double* __restrict__ F, int64_t rows_pad, int rows, int k, double x, double lam,
                                                            double* __restrict__ S, double* __restrict__ D) {
    const int64_t total = rows_pad * BMF_TW_KC;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / BMF_TW_KC;
        const int j = (int)(i - r * BMF_TW_KC);
        double s = 0.0, d = 0.0;
        if (r < rows && j < k) sigmoid_pair_mw((F[i] - x) * lam, lam, s, d);
        S[i] = s;
        if (D) D[i] = d;
    }
}

template <int CTRL>
__device__ __forceinline__ double mw_dpp_f64(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
// sum over the 64 lanes, in every lane (as group_sum<64> of thresh64.hip)
__device__ __forceinline__ double mw_wave_all(double v) {
    v += mw_dpp_f64<0xB1>(v);    // quad_perm [1, 0, 3, 2]
    v += mw_dpp_f64<0x4E>(v);    // quad_perm [2, 3, 0, 1]
    v += mw_dpp_f64<0x141>(v);   // row_half_mirror
    v += mw_dpp_f64<0x140>(v);   // row_mirror: the 16-lane row's sum
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// masked64_kernel of thresh64.hip at 128 columns: the cell list of a segment (<= 64 cells of one row) is one vector load (lane = cell);
// the whole wave takes one cell per step, lane l columns 2 l, 2 l + 1, four cells' gathers in flight; the dot product of a cell runs
// over all 128 columns (two FMAs per lane, then the sum over the lanes) before the residual is formed.
// partial[block][0..2] = sum (w r)^2, sum w r <dUs_i, Vs_j>, sum w r <Us_i, dVs_j> over the block's cells.
template <bool GRAD>
__global__ __launch_bounds__(256) void mw_cells_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const float* __restrict__ val,
                                                        const float* __restrict__ wgt, const int32_t* __restrict__ seg_row,
                                                        const int64_t* __restrict__ seg_beg, int nseg, const double* __restrict__ Us,
                                                        const double* __restrict__ dUs, const double* __restrict__ Vs, const double* __restrict__ dVs,
                                                        double* __restrict__ partial) {
    constexpr int NQ = 4;
    __shared__ double red[4][3];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const f64x2 zero = {0.0, 0.0};
    double f = 0.0, g1 = 0.0, g2 = 0.0;   // the same in every lane
    for (int sg = blockIdx.x * 4 + wave; sg < nseg; sg += gridDim.x * 4) {
        const int r = seg_row[sg];
        const int64_t base = seg_beg[sg];
        const int cnt = (int)min((int64_t)64, ptr[r + 1] - base);
        const f64x2 u = *reinterpret_cast<const f64x2*>(Us + (int64_t)r * BMF_TW_KC + 2 * lane);
        const f64x2 du = GRAD ? *reinterpret_cast<const f64x2*>(dUs + (int64_t)r * BMF_TW_KC + 2 * lane) : zero;
        const int64_t me = base + min(lane, cnt - 1);
        const int my_j = idx[me];
        const float my_x = val[me];
        const float my_w = wgt ? wgt[me] : 1.f;
        for (int q0 = 0; q0 < cnt; q0 += NQ) {
            double x[NQ], w[NQ];
            f64x2 v[NQ], dv[GRAD ? NQ : 1];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int cell = q0 + q;
                const int qq = min(cell, cnt - 1);   // tail: repeat the last cell with weight 0
                const int j = __builtin_amdgcn_readlane(my_j, qq);
                x[q] = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_x), qq));
                const float wq = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), qq));
                w[q] = cell < cnt ? (double)wq : 0.0;
                v[q] = *reinterpret_cast<const f64x2*>(Vs + (int64_t)j * BMF_TW_KC + 2 * lane);
                if (GRAD) dv[q] = *reinterpret_cast<const f64x2*>(dVs + (int64_t)j * BMF_TW_KC + 2 * lane);
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const double rr = w[q] * (x[q] - mw_wave_all(fma(u.y, v[q].y, u.x * v[q].x)));
                f += rr * rr;
                if (GRAD) {
                    g1 += rr * mw_wave_all(fma(du.y, v[q].y, du.x * v[q].x));
                    g2 += rr * mw_wave_all(fma(u.y, dv[q].y, u.x * dv[q].x));
                }
            }
        }
    }
    if (lane == 0) { red[wave][0] = f; red[wave][1] = g1; red[wave][2] = g2; }
    __syncthreads();
    if (threadIdx.x < 3) partial[(int64_t)blockIdx.x * 4 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// out[c] = sum_b partial[b][c], c < 3, in a fixed order (sum_partials_kernel of thresh64.hip)
__global__ __launch_bounds__(1024) void mw_sum_partials_kernel(const double* __restrict__ partial, int64_t nblk, double* __restrict__ out) {
    __shared__ double red[4][256];
    const int c = threadIdx.x & 3, q = threadIdx.x >> 2;
    double acc = 0.0;
    if (c < 3)
        for (int64_t b = q; b < nblk; b += 256) acc += partial[b * 4 + c];
    red[c][q] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (q < o) red[c][q] += red[c][q + o];
        __syncthreads();
    }
    if (q == 0 && c < 3) out[c] = red[c][0];
}

}  // namespace

#define BMF_TW_RANK(who, narrow) \
    BMF_REQUIRE(k > 64 && k <= BMF_TW_KC, who ": k=%d outside 65..128 (k <= 64: " narrow "; this build supports k <= 128)", k)

extern "C" int bmf_thresh_trace_wide_max_pairs(int k) {
    BMF_TW_RANK("bmf_thresh_trace_wide_max_pairs", "bmf_thresh_trace64_max_pairs");
    return BMF_TW_MAX_PAIRS;
}

// doubles of workspace for up to max_pairs pairs; the first word is the completion counter of the final kernel
extern "C" int64_t bmf_thresh_trace_wide_work(int32_t m, int32_t n, int k, int max_pairs) {
    BMF_TW_RANK("bmf_thresh_trace_wide_work", "bmf_thresh_trace64_work");
    BMF_REQUIRE(m >= 1 && n >= 1, "bmf_thresh_trace_wide_work: bad shape");
    BMF_REQUIRE(max_pairs >= 1 && max_pairs <= BMF_TW_MAX_PAIRS, "bmf_thresh_trace_wide_work: max_pairs=%d outside 1..%d", max_pairs, BMF_TW_MAX_PAIRS);
    const int64_t pa = max_pairs, mrows = (int64_t)m + 1, nrows = (int64_t)n + 1;
    const int64_t uch = tw_chunks(mrows), vch = tw_chunks(nrows), cmax = uch > vch ? uch : vch;
    return 2 + 2 * pa * (mrows + nrows) * BMF_TW_KC + BMF_TW_MAX_SEGMENTS(m) * pa * 3 + 4 * pa * cmax * BMF_TW_KC * BMF_TW_KC;
}

extern "C" int bmf_thresh_trace_wide(const int32_t* seg_row, const int64_t* seg_beg, const int32_t* seg_len, int32_t nseg, const int32_t* idx, int32_t m,
                                     int32_t n, const double* U64, const double* V64, int64_t ldf, int k, const double* uv_host, int32_t n_pairs,
                                     double lamda, double sum_x, int want_grad, double* work, double* out_host, double seq, void* stream) {
    BMF_REQUIRE(seg_row && seg_beg && seg_len && idx && U64 && V64 && uv_host && work && out_host, "bmf_thresh_trace_wide: null pointer");
    BMF_REQUIRE(bmf_aligned16(work), "bmf_thresh_trace_wide: work must be 16-byte aligned");
    BMF_TW_RANK("bmf_thresh_trace_wide", "bmf_thresh_trace64");
    BMF_REQUIRE(m >= 1 && n >= 1 && ldf >= k, "bmf_thresh_trace_wide: bad shape");
    BMF_REQUIRE(nseg >= 1 && nseg <= BMF_TW_MAX_SEGMENTS(m), "bmf_thresh_trace_wide: nseg=%d outside 1..%lld", nseg, (long long)BMF_TW_MAX_SEGMENTS(m));
    BMF_REQUIRE(n_pairs >= 1 && n_pairs <= BMF_TW_MAX_PAIRS, "bmf_thresh_trace_wide: n_pairs=%d outside 1..%d for k=%d", n_pairs, BMF_TW_MAX_PAIRS, k);
    hipStream_t s = (hipStream_t)stream;
    const int pa = n_pairs;
    const int64_t mrows = (int64_t)m + 1, nrows = (int64_t)n + 1;
    BMF_REQUIRE(mrows * BMF_TW_KC < (1ll << 31) && nrows * BMF_TW_KC < (1ll << 31), "bmf_thresh_trace_wide: factor too large");
    const int uch = tw_chunks(mrows), vch = tw_chunks(nrows);
    WidePairs pr;
    for (int p = 0; p < BMF_TW_MAX_PAIRS; ++p) {   // (slots past n_pairs repeat the last pair; they are never used)
        const int q = p < n_pairs ? p : n_pairs - 1;
        pr.u[p] = uv_host[2 * q];
        pr.v[p] = uv_host[2 * q + 1];
    }
    // the layout follows the pairs of THIS call (it fits whatever max_pairs >= n_pairs the workspace was sized for)
    unsigned* counter = reinterpret_cast<unsigned*>(work);
    double* Us = work + 2;
    double* dUs = Us + (int64_t)pa * mrows * BMF_TW_KC;
    double* Vs = dUs + (int64_t)pa * mrows * BMF_TW_KC;
    double* dVs = Vs + (int64_t)pa * nrows * BMF_TW_KC;
    double* cellpart = dVs + (int64_t)pa * nrows * BMF_TW_KC;
    double* grampart = cellpart + (((int64_t)nseg * pa * 3 + 1) & ~(int64_t)1);   // (16-byte aligned: the Gram tiles are written two doubles at a time)
    int gu = (int)((mrows * BMF_TW_KC + 255) / 256), gv = (int)((nrows * BMF_TW_KC + 255) / 256);
    if (gu > 1024) gu = 1024;
    if (gv > 1024) gv = 1024;
    BMF_LAUNCH(tw_transform_kernel, dim3((unsigned)(gu + gv), (unsigned)pa), dim3(256), 0, s, U64, ldf, m, mrows, V64, n, nrows, k, lamda, pr, Us,
               want_grad ? dUs : nullptr, Vs, want_grad ? dVs : nullptr, gu);
    const int gram_blocks = pa * (want_grad ? 2 : 1) * (uch + vch);
    BMF_LAUNCH(tw_gram_kernel, dim3((unsigned)gram_blocks), dim3(256), 0, s, mrows, nrows, pa, want_grad, Us, dUs, Vs, dVs, grampart, uch, vch);
    const unsigned cell_blocks = (unsigned)((nseg + 3) / 4);
    for (int g0 = 0; g0 < pa; g0 += 2) {   // two pairs per pass (header)
        const int gq = pa - g0 < 2 ? pa - g0 : 2;
        const double* us = Us + (int64_t)g0 * mrows * BMF_TW_KC;
        const double* dus = dUs + (int64_t)g0 * mrows * BMF_TW_KC;
        const double* vs = Vs + (int64_t)g0 * nrows * BMF_TW_KC;
        const double* dvs = dVs + (int64_t)g0 * nrows * BMF_TW_KC;
        double* cpart = cellpart + (int64_t)g0 * 3 * nseg;
        if (want_grad) {
            if (gq == 1) BMF_LAUNCH((tw_cells_kernel<true, 1>), dim3(cell_blocks), dim3(256), 0, s, seg_row, seg_beg, seg_len, idx, nseg, mrows, nrows, gq, us, dus, vs, dvs, cpart);
            else BMF_LAUNCH((tw_cells_kernel<true, 2>), dim3(cell_blocks), dim3(256), 0, s, seg_row, seg_beg, seg_len, idx, nseg, mrows, nrows, gq, us, dus, vs, dvs, cpart);
        } else {
            if (gq == 1) BMF_LAUNCH((tw_cells_kernel<false, 1>), dim3(cell_blocks), dim3(256), 0, s, seg_row, seg_beg, seg_len, idx, nseg, mrows, nrows, gq, us, dus, vs, dvs, cpart);
            else BMF_LAUNCH((tw_cells_kernel<false, 2>), dim3(cell_blocks), dim3(256), 0, s, seg_row, seg_beg, seg_len, idx, nseg, mrows, nrows, gq, us, dus, vs, dvs, cpart);
        }
    }
    BMF_LAUNCH(tw_final_kernel, dim3((unsigned)n_pairs), dim3(1024), 0, s, cellpart, grampart, nseg, n_pairs, uch, vch, sum_x, want_grad, out_host, seq, counter);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_thresh_transform64_wide(const double* F, int64_t rows_pad, int32_t rows, int k, double x, double lamda, double* S, double* D,
                                           void* stream) {
    BMF_REQUIRE(F && S, "bmf_thresh_transform64_wide: null pointer");
    BMF_TW_RANK("bmf_thresh_transform64_wide", "bmf_thresh_transform64");
    BMF_REQUIRE(rows >= 1 && rows <= rows_pad, "bmf_thresh_transform64_wide: bad shape");
    const int64_t g = (rows_pad * BMF_TW_KC + 255) / 256;
    BMF_LAUNCH(mw_transform_kernel, dim3((unsigned)(g < 2048 ? g : 2048)), dim3(256), 0, (hipStream_t)stream, F, rows_pad, rows, k, x, lamda, S, D);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_masked_thresh64_wide(const int64_t* ptr, const int32_t* idx, const float* val, const float* wgt, const int32_t* seg_row,
                                        const int64_t* seg_beg, int32_t nseg, const double* Us, const double* dUs, const double* Vs, const double* dVs,
                                        int k, double* partial, int32_t partial_blocks, double* out, void* stream) {
    BMF_REQUIRE(ptr && idx && val && seg_row && seg_beg && Us && Vs && partial && out, "bmf_masked_thresh64_wide: null pointer");
    BMF_REQUIRE((dUs == nullptr) == (dVs == nullptr), "bmf_masked_thresh64_wide: give both derivative factors or neither");
    BMF_REQUIRE(bmf_aligned16(Us) && bmf_aligned16(dUs) && bmf_aligned16(Vs) && bmf_aligned16(dVs), "bmf_masked_thresh64_wide: the transformed factors must be 16-byte aligned");
    BMF_TW_RANK("bmf_masked_thresh64_wide", "bmf_masked_thresh64_k");
    BMF_REQUIRE(nseg >= 1 && partial_blocks >= 1 && partial_blocks <= 65535, "bmf_masked_thresh64_wide: bad nseg / partial_blocks");
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)partial_blocks), block(256);
    if (dUs) BMF_LAUNCH(mw_cells_kernel<true>, grid, block, 0, s, ptr, idx, val, wgt, seg_row, seg_beg, nseg, Us, dUs, Vs, dVs, partial);
    else BMF_LAUNCH(mw_cells_kernel<false>, grid, block, 0, s, ptr, idx, val, wgt, seg_row, seg_beg, nseg, Us, dUs, Vs, dVs, partial);
    BMF_LAUNCH(mw_sum_partials_kernel, dim3(1), dim3(1024), 0, s, partial, (int64_t)partial_blocks, out);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}
