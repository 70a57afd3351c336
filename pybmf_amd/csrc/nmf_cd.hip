// Coordinate-descent NMF (scikit-learn's Frobenius 'cd' solver, the solver behind PyBMF/models/NMFSklearn.py): the sweep over the
// rows of one factor, and one whole iteration of the solver as a chain of launches.
//
// The sweep is _update_cdnmf_fast(W, HHt, XHt, arange(k)) restated: inside a row the coordinates t = 0 .. k-1 are updated one after
// the other (Gauss-Seidel: the gradient of coordinate t sees the new values of the coordinates before it), rows are independent.
// One lane owns one row and keeps it in registers (kp fp64 values: 128 VGPRs at kp = 64); a workgroup of two waves owns the 128 rows
// of one block of the column maxima.  HHt sits in the LDS, where all lanes read the same address at the same time (a broadcast); the
// row of W and the numerators XHt travel through a 128 x 16 staging tile in the LDS, so that global loads and stores are row pieces
// of 64 to 128 bytes and a lane then reads its own row of the tile (row stride 17 doubles: conflict-free 8-byte reads).
//
// The coordinate loop is a run-time loop inside each group of 16 coordinates (the group index is unrolled): the lane's register of
// coordinate t is picked and rewritten by a chain of 16 selects, the 64 products of the gradient address registers at compile time.
// A full unroll over t as well would be 4096 multiply-add pairs of straight-line code at kp = 64, larger than the instruction cache.
//
// Arithmetic is fp64 in the reference's order, one product and one sum per term (this file is built with -ffp-contract=off).
#include "common.h"

namespace {

constexpr int NMF_ROWS = 128;          // rows per workgroup = one block of the column maxima
constexpr int NMF_Q = 16;              // coordinates per staged group
constexpr int NMF_LD = NMF_Q + 1;      // row stride of the staging tile, in doubles

template <int KP>
__global__ __launch_bounds__(NMF_ROWS, 2) void nmf_cd_sweep_kernel(double* __restrict__ F64, float* __restrict__ F, int rows, int k,
                                                                    const float* __restrict__ num, int64_t slab_stride, int splits,
                                                                    const double* __restrict__ G, float* __restrict__ blockmax,
                                                                    double* __restrict__ viol) {
    __shared__ __attribute__((aligned(16))) double sG[KP * KP];
    __shared__ double tile[NMF_ROWS * NMF_LD];
    __shared__ float smax[NMF_ROWS / 8][NMF_Q];
    __shared__ double sred[NMF_ROWS / 64];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * NMF_ROWS;

    // HHt; what lies beyond k is not read and counts as zero (its products with the zero padding of W then add exact zeros)
    for (int e = tid; e < KP * KP; e += NMF_ROWS) sG[e] = (e / KP < k && e % KP < k) ? G[e] : 0.0;

    // the lane's row of W: group by group through the tile; thread -> (row c / 8, column pair c % 8) of a group, c = tid + 128 u
    double w[KP];
#pragma unroll
    for (int q = 0; q < KP / NMF_Q; ++q) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = tid + NMF_ROWS * u, rr = c >> 3, cp = (c & 7) * 2, col = q * NMF_Q + cp;
            const double2 v = *reinterpret_cast<const double2*>(F64 + (r0 + rr) * KP + col);
            const bool live = r0 + rr < rows;
            tile[rr * NMF_LD + cp] = (live && col < k) ? v.x : 0.0;
            tile[rr * NMF_LD + cp + 1] = (live && col + 1 < k) ? v.y : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NMF_Q; ++j) w[q * NMF_Q + j] = tile[tid * NMF_LD + j];
    }

    double vio = 0.0;
#pragma unroll
    for (int q = 0; q < KP / NMF_Q; ++q) {
        if (q * NMF_Q >= k) break;   // (the same in every lane)
        // XHt of this group: the slabs added in fp64 in slab order; thread -> (row c / 4, four columns c % 4), c = tid + 128 u
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = tid + NMF_ROWS * u, rr = c >> 2, c4 = (c & 3) * 4, col = q * NMF_Q + c4;
            double x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0;
            if (r0 + rr < rows && col < k) {
                const float* p = num + (r0 + rr) * KP + col;
                if (col + 4 <= k) {
                    for (int s = 0; s < splits; ++s) {
                        const float4 v = *reinterpret_cast<const float4*>(p + (int64_t)s * slab_stride);
                        x0 += (double)v.x; x1 += (double)v.y; x2 += (double)v.z; x3 += (double)v.w;
                    }
                } else {   // the group k ends in: nothing beyond column k - 1 is read
                    for (int s = 0; s < splits; ++s) {
                        const float* ps = p + (int64_t)s * slab_stride;
                        x0 += (double)ps[0];
                        if (col + 1 < k) x1 += (double)ps[1];
                        if (col + 2 < k) x2 += (double)ps[2];
                    }
                }
            }
            double* d = tile + rr * NMF_LD + c4;
            d[0] = x0; d[1] = x1; d[2] = x2; d[3] = x3;
        }
        __syncthreads();
        const int jn = min(NMF_Q, k - q * NMF_Q);
#pragma unroll 1
        for (int j = 0; j < jn; ++j) {
            const int t = q * NMF_Q + j;
            const double* g = sG + t * KP;
            const double2* g2 = reinterpret_cast<const double2*>(g);
            double grad = -tile[tid * NMF_LD + j];
            // row t of HHt in pieces of 16, the next piece on its way while this one is used; the fences keep the scheduler from
            // fetching the whole row ahead (128 registers at kp = 64, on top of the 128 of the lane's row of W)
            double2 gb[2][8];
#pragma unroll
            for (int i = 0; i < 8; ++i) gb[0][i] = g2[i];
#pragma unroll
            for (int c = 0; c < KP / 16; ++c) {
                __builtin_amdgcn_sched_barrier(0);
                if (c + 1 < KP / 16) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) gb[(c + 1) & 1][i] = g2[8 * (c + 1) + i];
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    grad += gb[c & 1][i].x * w[16 * c + 2 * i];
                    grad += gb[c & 1][i].y * w[16 * c + 2 * i + 1];
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            double old = w[q * NMF_Q];
#pragma unroll
            for (int jj = 1; jj < NMF_Q; ++jj) old = (j == jj) ? w[q * NMF_Q + jj] : old;
            const double pg = (old == 0.0) ? (grad < 0.0 ? grad : 0.0) : grad;
            vio += fabs(pg);
            const double hess = g[t];
            if (hess != 0.0) {   // (the same in every lane)
                double nw = old - grad / hess;
                nw = (0.0 > nw) ? 0.0 : nw;
#pragma unroll
                for (int jj = 0; jj < NMF_Q; ++jj) w[q * NMF_Q + jj] = (j == jj) ? nw : w[q * NMF_Q + jj];
            }
        }
    }

    // the violation of the block: lanes by the butterfly of wave_sum, then the waves in order
    vio = wave_sum(vio);
    if ((tid & 63) == 0) sred[tid >> 6] = vio;

    // the new rows: fp64, the fp32 shadow and the column maxima of the shadow, group by group through the tile
#pragma unroll
    for (int q = 0; q < KP / NMF_Q; ++q) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NMF_Q; ++j) tile[tid * NMF_LD + j] = w[q * NMF_Q + j];
        __syncthreads();
        float m0 = 0.f, m1 = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = tid + NMF_ROWS * u, rr = c >> 3, cp = (c & 7) * 2, col = q * NMF_Q + cp;
            const double v0 = tile[rr * NMF_LD + cp], v1 = tile[rr * NMF_LD + cp + 1];
            const float f0 = (float)v0, f1 = (float)v1;
            *reinterpret_cast<double2*>(F64 + (r0 + rr) * KP + col) = make_double2(v0, v1);
            *reinterpret_cast<float2*>(F + (r0 + rr) * KP + col) = make_float2(f0, f1);
            m0 = fmaxf(m0, fabsf(f0));
            m1 = fmaxf(m1, fabsf(f1));
        }
        // (the thread's eight rows are (tid >> 3) + 16 u: sixteen threads share a column pair)
        smax[tid >> 3][(tid & 7) * 2] = m0;
        smax[tid >> 3][(tid & 7) * 2 + 1] = m1;
        __syncthreads();
        if (tid < NMF_Q) {
            float m = smax[0][tid];
#pragma unroll
            for (int gidx = 1; gidx < NMF_ROWS / 8; ++gidx) m = fmaxf(m, smax[gidx][tid]);
            blockmax[(int64_t)blockIdx.x * KP + q * NMF_Q + tid] = m;
        }
    }
    if (tid == 0) viol[blockIdx.x] = sred[0] + sred[1];
}

// out[0] = sum pu[0 .. nu), out[1] = sum pv[0 .. nv): the two violations of one iteration, in a fixed order
__global__ __launch_bounds__(256) void nmf_violations_kernel(const double* __restrict__ pu, int nu, const double* __restrict__ pv, int nv,
                                                              double* __restrict__ out) {
    __shared__ double red[2][4];
    const int t = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int i = t; i < nu; i += 256) a += pu[i];
    for (int i = t; i < nv; i += 256) b += pv[i];
    a = wave_sum(a);
    b = wave_sum(b);
    if ((t & 63) == 0) { red[0][t >> 6] = a; red[1][t >> 6] = b; }
    __syncthreads();
    if (t < 2) out[t] = ((red[t][0] + red[t][1]) + red[t][2]) + red[t][3];
}

}  // namespace

extern "C" int bmf_nmf_cd_sweep(double* F64, float* F, int64_t rows_pad, int32_t rows, int k, int kp, const float* num, int64_t slab_stride,
                                int splits, const double* G64, float* blockmax, double* viol, void* stream) {
    BMF_REQUIRE(F64 && F && num && G64 && blockmax && viol, "bmf_nmf_cd_sweep: null pointer");
    BMF_REQUIRE(rows_pad > 0 && rows_pad % NMF_ROWS == 0 && rows_pad / NMF_ROWS <= 0x7fffffff, "bmf_nmf_cd_sweep: rows_pad=%lld must be a positive multiple of 128",
                (long long)rows_pad);
    BMF_REQUIRE(rows >= 1 && rows <= rows_pad, "bmf_nmf_cd_sweep: rows=%d out of range", rows);
    BMF_REQUIRE((kp == 32 || kp == 64) && k >= 1 && k <= kp, "bmf_nmf_cd_sweep: need 1 <= k <= kp, kp in {32, 64} (k=%d, kp=%d)", k, kp);
    BMF_REQUIRE(splits >= 1 && slab_stride >= rows_pad * kp && slab_stride % 4 == 0, "bmf_nmf_cd_sweep: bad slab description");
    BMF_REQUIRE(bmf_aligned16(F64) && bmf_aligned16(F) && bmf_aligned16(num), "bmf_nmf_cd_sweep: F64, F and num must be 16-byte aligned");
    const dim3 grid((unsigned)(rows_pad / NMF_ROWS)), block(NMF_ROWS);
    hipStream_t s = (hipStream_t)stream;
    if (kp == 32) BMF_LAUNCH(nmf_cd_sweep_kernel<32>, grid, block, 0, s, F64, F, rows, k, num, slab_stride, splits, G64, blockmax, viol);
    else BMF_LAUNCH(nmf_cd_sweep_kernel<64>, grid, block, 0, s, F64, F, rows, k, num, slab_stride, splits, G64, blockmax, viol);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

// ---- one iteration per call (bmf_nmf_state) ------------------------------------------------------------------------------------------
int bmf_panel_i8_launch(const double* F64, const float* F, int64_t rows_pad, int64_t ldf, int kp, int limbs, int8_t* panel, int64_t ldp,
                        float* ws, float* scale, bool have_blockmax, const int32_t* stop, hipStream_t s, bool have_scale,
                        const float* flags, float* colscale_out, const float* rslabs, int rcount, int rn, float* rout32, double* rout64);

static int nmf_check_state(const bmf_nmf_state* st, int it) {
    BMF_REQUIRE(st, "bmf_nmf_cd_iterate: null state");
    BMF_REQUIRE(st->struct_bytes == (int32_t)sizeof(bmf_nmf_state), "bmf_nmf_cd_iterate: struct_bytes=%d, library expects %d", st->struct_bytes,
                (int)sizeof(bmf_nmf_state));
    BMF_REQUIRE(st->Xtiled && st->XTtiled && st->U64 && st->V64 && st->U && st->V && st->Upanel && st->Vpanel && st->scaleU && st->scaleV && st->wsU &&
                    st->wsV && st->Mslab && st->Nslab && st->gram_slabs && st->GU && st->GV && st->GU64 && st->GV64 && st->partU && st->partV && st->log,
                "bmf_nmf_cd_iterate: null pointer in the state");
    BMF_REQUIRE(st->m_pad > 0 && st->n_pad > 0 && st->m_pad % 512 == 0 && st->n_pad % 512 == 0, "bmf_nmf_cd_iterate: m_pad, n_pad must be multiples of 512");
    BMF_REQUIRE(st->m >= 1 && st->m <= st->m_pad && st->n >= 1 && st->n <= st->n_pad, "bmf_nmf_cd_iterate: m, n out of range");
    BMF_REQUIRE((st->kp == 32 || st->kp == 64) && st->k >= 1 && st->k <= st->kp, "bmf_nmf_cd_iterate: need 1 <= k <= kp, kp in {32, 64}");
    BMF_REQUIRE(st->splits_xv >= 1 && st->splits_xtu >= 1 && st->gram_blocks >= 1, "bmf_nmf_cd_iterate: splits and gram_blocks must be >= 1");
    BMF_REQUIRE(st->log_rows >= 1 && it >= 0, "bmf_nmf_cd_iterate: need log_rows >= 1 and it >= 0");
    return BMF_OK;
}

extern "C" int bmf_nmf_cd_iterate(const bmf_nmf_state* st, int it, void* stream) {
    int rc = nmf_check_state(st, it);
    if (rc != BMF_OK) return rc;
    const int kp = st->kp, kk = kp * kp;
    hipStream_t s = (hipStream_t)stream;
    for (int side = 0; side < 2; ++side) {
        const bool u_side = side == 0;
        // the factor that moves (F) and the one that is held (H): W, Ht of _update_coordinate_descent(X, W, Ht) / (X^T, Ht, W)
        const int64_t rows_pad = u_side ? st->m_pad : st->n_pad, held_pad = u_side ? st->n_pad : st->m_pad;
        const float* H = u_side ? st->V : st->U;
        float* GH = u_side ? st->GV : st->GU;
        double* GH64 = u_side ? st->GV64 : st->GU64;
        float* slab = u_side ? st->Mslab : st->Nslab;
        const int splits = u_side ? st->splits_xv : st->splits_xtu;
        double* F64 = u_side ? st->U64 : st->V64;
        float* F = u_side ? st->U : st->V;
        float* ws = u_side ? st->wsU : st->wsV;
        if ((rc = bmf_gram_partial(H, held_pad, kp, kp, st->gram_slabs, st->gram_blocks, stream)) != BMF_OK) return rc;
        if ((rc = bmf_reduce_slabs(st->gram_slabs, kk, st->gram_blocks, kk, GH, GH64, stream)) != BMF_OK) return rc;
        rc = bmf_xf_bits_i8(u_side ? st->Xtiled : st->XTtiled, rows_pad, held_pad / 32, held_pad / 32, u_side ? st->Vpanel : st->Upanel, held_pad, 3,
                            (u_side ? st->scaleV : st->scaleU) + kp, kp, slab, rows_pad * kp, splits, 1, stream);
        if (rc != BMF_OK) return rc;
        bmf_timer_begin(s);
        rc = bmf_nmf_cd_sweep(F64, F, rows_pad, u_side ? st->m : st->n, st->k, kp, slab, rows_pad * kp, splits, GH64, ws, u_side ? st->partU : st->partV,
                              stream);
        bmf_timer_end(s);
        if (rc != BMF_OK) return rc;
        // the digit planes of the new factor, from the block maxima the sweep left in ws (bmf_make_panel_i8 without its own maxima pass)
        rc = bmf_panel_i8_launch(F64, F, rows_pad, kp, kp, 3, u_side ? st->Upanel : st->Vpanel, rows_pad, ws, u_side ? st->scaleU : st->scaleV, true, nullptr, s,
                                 false, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr);
        if (rc != BMF_OK) return rc;
    }
    BMF_LAUNCH(nmf_violations_kernel, dim3(1), dim3(256), 0, s, st->partU, (int)(st->m_pad / NMF_ROWS), st->partV, (int)(st->n_pad / NMF_ROWS),
               st->log + 8 * (int64_t)(it % st->log_rows));
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}
