// The link passes of csrc/link.hip for a rank 64 < k <= 128 (PNLPF and WNMF with the Kullback-Leibler loss; the reference has no rank
// limit, PyBMF/models/PNLPF.py:61-91, WNMF.py:111-129).  A factor is two blocks of 64 columns, F = [F_0 | F_1], fp32 [rows_pad][64] each,
// zero padded (pybmf_amd/wide.py).  The two-block trick of wide.py does not carry over: the non-linearity is applied to the WHOLE dot
// product P = sum_b F_self,b F_other,b^T, before anything is contracted again, so P cannot be formed per block.  Per 32 x 32 tile:
//   1. P^T on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) over both blocks: 64 steps, block 0 first.  Sigmoid link: every step starts
//      from zero and the steps are added in fp64, as link_pass_kernel does and for its reason (lamda multiplies the rounding of a P near 1/2);
//   2. g1 / g2 element-wise in registers, masked by rows / cols as in link_pass_kernel;
//   3. out_b += g F_other,b for block 0, then for block 1, FROM THE SAME g: the C/D registers of step 1 are the A operand of step 3, the
//      B operand of step s is row j0 + jr(s, h) of the block -- its 16 x 2 loads are requested per block, so the two blocks share the
//      registers that hold them.
// One wave per 32 rows, four waves per workgroup, all eight accumulators (2 blocks x 2 column tiles x {num, den}) in registers over the
// sweep of j; one wave per SIMD.  A correctness row like the other wide ranks: no 16-bit-MFMA flavour, no one-C-call loop.
#include "common.h"

namespace {

constexpr int BK = 64;        // columns of a block
constexpr int KH = BK / 2;    // MFMA steps of P per block (two products each)
constexpr int NT = BK / 32;   // 32-column tiles of a block

__device__ __forceinline__ void sigmoid_parts(float s, float& sig, float& d) {
    // sig = sigmoid(s), d = sig (1 - sig) without cancellation: with e = exp(-|s|), d = e / (1 + e)^2   (as in link.hip)
    const float e = __expf(-fabsf(s));
    const float r = __builtin_amdgcn_rcpf(1.0f + e);
    sig = s >= 0.f ? r : e * r;
    d = e * r * r;
}

__device__ __forceinline__ void load_half_row(const float* __restrict__ p, float (&v)[KH]) {
#pragma unroll
    for (int s = 0; s < KH; s += 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p + s);
        v[s] = q[0]; v[s + 1] = q[1]; v[s + 2] = q[2]; v[s + 3] = q[3];
    }
}

template <int LINK>
__global__ __launch_bounds__(256) void link_pass_wide_kernel(const uint32_t* __restrict__ Xbits, int64_t ldx, int rows, int cols,
                                                              const float* __restrict__ A0, const float* __restrict__ A1,
                                                              const float* __restrict__ B0, const float* __restrict__ B1, float lam,
                                                              int col_tiles_per_block, float* __restrict__ num0, float* __restrict__ num1,
                                                              float* __restrict__ den0, float* __restrict__ den1, int64_t slab_stride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    const int64_t i0 = ((int64_t)blockIdx.x * 4 + wave) * 32;  // 32 rows of X per wave
    const int col_tiles = (cols + 31) / 32;
    const int jt0 = blockIdx.y * col_tiles_per_block;
    const int jt1 = min(jt0 + col_tiles_per_block, col_tiles);

    float a0[KH], a1[KH];   // this lane's row of F_self: columns 32 h .. 32 h + 31 of each block
    load_half_row(A0 + (i0 + c) * BK + KH * h, a0);
    load_half_row(A1 + (i0 + c) * BK + KH * h, a1);
    const bool row_ok = (i0 + c) < rows;
    f32x16 o1[2][NT], o2[2][NT];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) { o1[b][nt][i] = 0.f; o2[b][nt][i] = 0.f; }

    for (int jt = jt0; jt < jt1; ++jt) {
        const int64_t j0 = (int64_t)jt * 32;
        const unsigned xw = Xbits[(i0 + c) * ldx + jt];
        f32x16 p;
#pragma unroll
        for (int i = 0; i < 16; ++i) p[i] = 0.f;
        double pd[16];
        if (LINK == BMF_LINK_SIGMOID) {
#pragma unroll
            for (int i = 0; i < 16; ++i) pd[i] = 0.0;
        }
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            float b[KH];
            load_half_row((blk ? B1 : B0) + (j0 + c) * BK + KH * h, b);
#pragma unroll
            for (int s = 0; s < KH; ++s) {
                const float as = blk ? a1[s] : a0[s];
                if (LINK == BMF_LINK_SIGMOID) {
                    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    const f32x16 step = __builtin_amdgcn_mfma_f32_32x32x2f32(b[s], as, zero, 0, 0, 0);
#pragma unroll
                    for (int i = 0; i < 16; ++i) pd[i] += (double)step[i];
                } else {
                    p = __builtin_amdgcn_mfma_f32_32x32x2f32(b[s], as, p, 0, 0, 0);
                }
            }
        }

        float g1[16], g2[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int jr = (i & 3) + 8 * (i >> 2) + 4 * h;
            const bool ok = row_ok && (j0 + jr) < cols;
            const bool x = (xw >> jr) & 1u;
            if (LINK == BMF_LINK_SIGMOID) {
                float sig, d;
                sigmoid_parts((float)((double)lam * (pd[i] - 0.5)), sig, d);
                g1[i] = (ok && x) ? lam * d : 0.f;
                g2[i] = ok ? lam * sig * d : 0.f;
            } else {
                g1[i] = (ok && x && p[i] > 0.f) ? __builtin_amdgcn_rcpf(p[i]) : 0.f;
                g2[i] = 0.f;
            }
        }
        // block 0, then block 1, from the same g: row j0 + jr(s, h) of the block, columns 32 nt + c
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const float* __restrict__ B = blk ? B1 : B0;
            float bv[16][NT];
#pragma unroll
            for (int s = 0; s < 16; ++s)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) bv[s][nt] = B[(j0 + (s & 3) + 8 * (s >> 2) + 4 * h) * BK + 32 * nt + c];
#pragma unroll
            for (int s = 0; s < 16; ++s)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    o1[blk][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(g1[s], bv[s][nt], o1[blk][nt], 0, 0, 0);
                    if (LINK == BMF_LINK_SIGMOID) o2[blk][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(g2[s], bv[s][nt], o2[blk][nt], 0, 0, 0);
                }
        }
    }
    // C/D layout: lane (c, h) holds column 32 nt + c of rows i0 + (reg & 3) + 8 (reg >> 2) + 4 h
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        float* on = (blk ? num1 : num0) + (int64_t)blockIdx.y * slab_stride;
        float* od = (blk ? den1 : den0);
        if (od) od += (int64_t)blockIdx.y * slab_stride;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t row = i0 + (i & 3) + 8 * (i >> 2) + 4 * h;
                on[row * BK + 32 * nt + c] = o1[blk][nt][i];
                if (LINK == BMF_LINK_SIGMOID && od) od[row * BK + 32 * nt + c] = o2[blk][nt][i];
            }
    }
}

// bmf_link_sums with P over both blocks: sums[0] += sum |x - f(p)|, sums[1] += sum (x - f(p))^2, sums[2] += the KL objective over the
// observed cells (link_sums_kernel's arithmetic, fp32 P)
template <int LINK>
__global__ __launch_bounds__(256) void link_sums_wide_kernel(const uint32_t* __restrict__ Xbits, int64_t ldx, int rows, int cols,
                                                              const float* __restrict__ A0, const float* __restrict__ A1,
                                                              const float* __restrict__ B0, const float* __restrict__ B1, float lam,
                                                              int col_tiles_per_block, const uint32_t* __restrict__ Obits,
                                                              double* __restrict__ sums) {
    __shared__ double red[4][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    const int64_t i0 = ((int64_t)blockIdx.x * 4 + wave) * 32;
    const int col_tiles = (cols + 31) / 32;
    const int jt0 = blockIdx.y * col_tiles_per_block;
    const int jt1 = min(jt0 + col_tiles_per_block, col_tiles);
    float a0[KH], a1[KH];
    load_half_row(A0 + (i0 + c) * BK + KH * h, a0);
    load_half_row(A1 + (i0 + c) * BK + KH * h, a1);
    const bool row_ok = (i0 + c) < rows;
    double s_abs = 0.0, s_sq = 0.0, s_kl = 0.0;
    for (int jt = jt0; jt < jt1; ++jt) {
        const int64_t j0 = (int64_t)jt * 32;
        const unsigned xw = Xbits[(i0 + c) * ldx + jt];
        const unsigned ow = Obits ? Obits[(i0 + c) * ldx + jt] : 0xffffffffu;  // observed cells (KL objective only)
        f32x16 p;
#pragma unroll
        for (int i = 0; i < 16; ++i) p[i] = 0.f;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            float b[KH];
            load_half_row((blk ? B1 : B0) + (j0 + c) * BK + KH * h, b);
#pragma unroll
            for (int s = 0; s < KH; ++s) p = __builtin_amdgcn_mfma_f32_32x32x2f32(b[s], blk ? a1[s] : a0[s], p, 0, 0, 0);
        }
        float t_abs = 0.f, t_sq = 0.f, t_kl = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int jr = (i & 3) + 8 * (i >> 2) + 4 * h;
            const bool ok = row_ok && (j0 + jr) < cols;
            const float x = (float)((xw >> jr) & 1u);
            float f = p[i];
            if (LINK == BMF_LINK_SIGMOID) {
                float d;
                sigmoid_parts(lam * (p[i] - 0.5f), f, d);
            }
            const float r = ok ? x - f : 0.f;
            t_abs += fabsf(r);
            t_sq = fmaf(r, r, t_sq);
            if (LINK == BMF_LINK_KL && ok && ((ow >> jr) & 1u)) t_kl += (x != 0.f) ? (p[i] - 1.0f - __logf(fmaxf(p[i], 1e-37f))) : p[i];
        }
        s_abs += (double)t_abs;
        s_sq += (double)t_sq;
        s_kl += (double)t_kl;
    }
    s_abs = wave_sum(s_abs);
    s_sq = wave_sum(s_sq);
    s_kl = wave_sum(s_kl);
    if (lane == 0) { red[wave][0] = s_abs; red[wave][1] = s_sq; red[wave][2] = s_kl; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int q = threadIdx.x;
        atomicAdd(&sums[q], ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q]);
    }
}

// masked_segments_wide_kernel (csrc/masked.hip) with the product sent through a link: p_e over both blocks, then per cell the sigmoid
// or the reciprocal exactly as masked_segments_kernel<64, LINK, 64> forms them, numerator / denominator partials per block.
template <int LINK>
__global__ __launch_bounds__(256) void masked_link_segments_wide_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                                         const float* __restrict__ val, const float* __restrict__ wgt,
                                                                         const int32_t* __restrict__ seg_row,
                                                                         const int64_t* __restrict__ seg_beg, int nseg,
                                                                         const float* __restrict__ Fself0, const float* __restrict__ Fself1,
                                                                         const float* __restrict__ Fother0, const float* __restrict__ Fother1,
                                                                         float* __restrict__ part0, float* __restrict__ part1,
                                                                         double* __restrict__ sums, float lamda) {
    __shared__ double red[4][2];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double s2 = 0.0, s1 = 0.0;
    for (int sg = blockIdx.x * 4 + wave; sg < nseg; sg += gridDim.x * 4) {
        const int r = seg_row[sg];
        const int64_t base = seg_beg[sg];
        const int cnt = (int)min((int64_t)64, ptr[r + 1] - base);
        const float u0 = Fself0[(int64_t)r * BK + lane], u1 = Fself1[(int64_t)r * BK + lane];
        const int64_t me = base + min(lane, cnt - 1);
        const int my_j = idx[me];
        const float my_x = val[me];
        const float my_w = wgt ? wgt[me] : 1.f;
        float n0 = 0.f, d0 = 0.f, n1 = 0.f, d1 = 0.f;
        for (int q0 = 0; q0 < cnt; q0 += 8) {
            float x[8], w[8], v0[8], v1[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int cell = q0 + q;
                const int qq = min(cell, cnt - 1);  // tail: repeat the last cell with weight 0
                const int j = __builtin_amdgcn_readlane(my_j, qq);
                x[q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_x), qq));
                w[q] = (cell < cnt) ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), qq)) : 0.f;
                v0[q] = Fother0[(int64_t)j * BK + lane];
                v1[q] = Fother1[(int64_t)j * BK + lane];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float p = wave_sum_dpp<64>(fmaf(u1, v1[q], u0 * v0[q]));   // (padding columns of both blocks hold 0)
                if constexpr (LINK == BMF_LINK_SIGMOID) {
                    const float sarg = lamda * (p - 0.5f);
                    const float e = __expf(-fabsf(sarg));            // sigma (1 - sigma) = e / (1 + e)^2 without cancellation
                    const float r1 = 1.0f / (1.0f + e);
                    const float pred = sarg >= 0.f ? r1 : e * r1;
                    const float dsig = e * r1 * r1;
                    const float cn = lamda * w[q] * x[q] * dsig, cd = lamda * w[q] * pred * dsig;
                    n0 = fmaf(cn, v0[q], n0);
                    d0 = fmaf(cd, v0[q], d0);
                    n1 = fmaf(cn, v1[q], n1);
                    d1 = fmaf(cd, v1[q], d1);
                    const double d = (double)x[q] - (double)pred;
                    s2 += (double)w[q] * d * d;
                    s1 += (double)w[q] * fabs(d);
                } else {
                    // Kullback-Leibler under a weight matrix: numerator (W o X / U V^T) F_other; the denominator is the caller's (column
                    // sums of F_other); sums[0] takes TWICE the objective, as masked_segments_kernel does
                    const float pp = fmaxf(p, 1e-30f);
                    const float cn = x[q] != 0.f ? w[q] * x[q] / pp : 0.f;
                    n0 = fmaf(cn, v0[q], n0);
                    n1 = fmaf(cn, v1[q], n1);
                    const double kl = (x[q] != 0.f ? (double)x[q] * log((double)x[q] / (double)pp) : 0.0) - (double)x[q] + (double)p;
                    s2 += 2.0 * (double)w[q] * kl;
                }
            }
        }
        part0[(int64_t)sg * 2 * BK + lane] = n0;
        part0[(int64_t)sg * 2 * BK + BK + lane] = d0;
        part1[(int64_t)sg * 2 * BK + lane] = n1;
        part1[(int64_t)sg * 2 * BK + BK + lane] = d1;
    }
    if (sums) {
        if (lane == 0) { red[wave][0] = s2; red[wave][1] = s1; }
        __syncthreads();
        if (threadIdx.x < 2) atomicAdd(&sums[threadIdx.x], ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x]);
    }
}

// num[r] / den[r] of one block = sum of the row's segment partials, in segment order (masked_rows_kernel of csrc/masked.hip)
__global__ __launch_bounds__(256) void masked_link_rows_wide_kernel(const int64_t* __restrict__ row_seg_ptr, int rows,
                                                                     const float* __restrict__ part, float* __restrict__ num,
                                                                     float* __restrict__ den) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int r = (int)(i / BK), c = (int)(i % BK);
    if (r >= rows) return;
    float a = 0.f, b = 0.f;
    const int64_t s1 = row_seg_ptr[r + 1];
    for (int64_t sg = row_seg_ptr[r]; sg < s1; ++sg) {
        a += part[sg * 2 * BK + c];
        b += part[sg * 2 * BK + BK + c];
    }
    num[i] = a;
    den[i] = b;
}

}  // namespace

#define BMF_LW_RANK(who, narrow) \
    BMF_REQUIRE(k > 64 && k <= 128, who ": k=%d outside 65..128 (k <= 64: " narrow "; this build supports k <= 128)", k)
#define BMF_LW_LINK(who) \
    BMF_REQUIRE(link == BMF_LINK_SIGMOID || link == BMF_LINK_KL, who ": link=%d, must be BMF_LINK_SIGMOID or BMF_LINK_KL", link)

extern "C" int bmf_link_pass_wide(const uint32_t* Xbits, int64_t rows_pad, int64_t ldx, int32_t rows, int32_t cols, const float* Fself0,
                                  const float* Fself1, const float* Fother0, const float* Fother1, int64_t other_pad, int k, int link,
                                  double lamda, float* num0, float* num1, float* den0, float* den1, int64_t slab_stride, int splits,
                                  void* stream) {
    BMF_REQUIRE(Xbits && Fself0 && Fself1 && Fother0 && Fother1 && num0 && num1, "bmf_link_pass_wide: null pointer");
    BMF_LW_RANK("bmf_link_pass_wide", "bmf_link_pass");
    BMF_LW_LINK("bmf_link_pass_wide");
    BMF_REQUIRE(link != BMF_LINK_SIGMOID || (den0 && den1), "bmf_link_pass_wide: the sigmoid link needs both den buffers");
    BMF_REQUIRE(rows >= 1 && cols >= 1 && rows <= rows_pad && rows_pad % 128 == 0, "bmf_link_pass_wide: bad rows/rows_pad");
    BMF_REQUIRE(cols <= other_pad && other_pad % 32 == 0 && ldx * 32 >= cols, "bmf_link_pass_wide: other_pad / ldx do not cover cols");
    const int want = bmf_link_splits(rows, cols);
    BMF_REQUIRE(splits == want, "bmf_link_pass_wide: splits=%d, this shape needs %d (bmf_link_splits)", splits, want);
    BMF_REQUIRE(slab_stride >= rows_pad * BK, "bmf_link_pass_wide: slab_stride too small");
    BMF_REQUIRE(bmf_aligned16(Fself0) && bmf_aligned16(Fself1) && bmf_aligned16(Fother0) && bmf_aligned16(Fother1),
                "bmf_link_pass_wide: factors must be 16-byte aligned");
    const int col_tiles = (cols + 31) / 32;
    const int per = (col_tiles + splits - 1) / splits;
    dim3 grid((unsigned)(rows_pad / 128), (unsigned)splits), block(256);
    hipStream_t s = (hipStream_t)stream;
    const float lam = (float)lamda;
    if (link == BMF_LINK_SIGMOID)
        BMF_LAUNCH((link_pass_wide_kernel<BMF_LINK_SIGMOID>), grid, block, 0, s, Xbits, ldx, rows, cols, Fself0, Fself1, Fother0, Fother1, lam, per,
                   num0, num1, den0, den1, slab_stride);
    else
        BMF_LAUNCH((link_pass_wide_kernel<BMF_LINK_KL>), grid, block, 0, s, Xbits, ldx, rows, cols, Fself0, Fself1, Fother0, Fother1, lam, per,
                   num0, num1, den0, den1, slab_stride);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_link_sums_wide(const uint32_t* Xbits, int64_t m_pad, int64_t ldx, int32_t m, int32_t n, const float* U0, const float* U1,
                                  const float* V0, const float* V1, int64_t n_pad, int k, int link, double lamda, const uint32_t* Obits,
                                  double* sums, void* stream) {
    BMF_REQUIRE(Xbits && U0 && U1 && V0 && V1 && sums, "bmf_link_sums_wide: null pointer");
    BMF_LW_RANK("bmf_link_sums_wide", "bmf_link_sums");
    BMF_LW_LINK("bmf_link_sums_wide");
    BMF_REQUIRE(m >= 1 && n >= 1 && m <= m_pad && m_pad % 128 == 0 && n <= n_pad && n_pad % 32 == 0 && ldx * 32 >= n,
                "bmf_link_sums_wide: bad shape");
    BMF_REQUIRE(bmf_aligned16(U0) && bmf_aligned16(U1) && bmf_aligned16(V0) && bmf_aligned16(V1),
                "bmf_link_sums_wide: factors must be 16-byte aligned");
    const int splits = bmf_link_splits(m, n);
    const int col_tiles = (n + 31) / 32;
    const int per = (col_tiles + splits - 1) / splits;
    dim3 grid((unsigned)((m + 127) / 128), (unsigned)splits), block(256);
    hipStream_t s = (hipStream_t)stream;
    const float lam = (float)lamda;
    if (link == BMF_LINK_SIGMOID)
        BMF_LAUNCH((link_sums_wide_kernel<BMF_LINK_SIGMOID>), grid, block, 0, s, Xbits, ldx, m, n, U0, U1, V0, V1, lam, per, Obits, sums);
    else
        BMF_LAUNCH((link_sums_wide_kernel<BMF_LINK_KL>), grid, block, 0, s, Xbits, ldx, m, n, U0, U1, V0, V1, lam, per, Obits, sums);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_masked_link_pass_wide(const int64_t* ptr, const int32_t* idx, const float* val, const float* wgt, int32_t rows,
                                         const int32_t* seg_row, const int64_t* seg_beg, int32_t nseg, const int64_t* row_seg_ptr,
                                         const float* Fself0, const float* Fself1, const float* Fother0, const float* Fother1, float* part0,
                                         float* part1, float* num0, float* num1, float* den0, float* den1, double* sums, int link,
                                         double lamda, void* stream) {
    BMF_REQUIRE(ptr && idx && val && seg_row && seg_beg && row_seg_ptr && Fself0 && Fself1 && Fother0 && Fother1 && part0 && part1 && num0 &&
                    num1 && den0 && den1,
                "bmf_masked_link_pass_wide: null pointer");
    BMF_REQUIRE(link != 0, "bmf_masked_link_pass_wide: link=0 is bmf_masked_pass_wide");
    BMF_LW_LINK("bmf_masked_link_pass_wide");
    BMF_REQUIRE(rows >= 1 && nseg >= 0, "bmf_masked_link_pass_wide: rows must be positive, nseg non-negative");
    hipStream_t s = (hipStream_t)stream;
    if (nseg > 0) {
        const int blocks = (nseg + 3) / 4;
        dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192)), block(256);
        if (link == BMF_LINK_SIGMOID)
            BMF_LAUNCH((masked_link_segments_wide_kernel<BMF_LINK_SIGMOID>), grid, block, 0, s, ptr, idx, val, wgt, seg_row, seg_beg, nseg, Fself0,
                       Fself1, Fother0, Fother1, part0, part1, sums, (float)lamda);
        else
            BMF_LAUNCH((masked_link_segments_wide_kernel<BMF_LINK_KL>), grid, block, 0, s, ptr, idx, val, wgt, seg_row, seg_beg, nseg, Fself0,
                       Fself1, Fother0, Fother1, part0, part1, sums, (float)lamda);
    }
    const int64_t total = (int64_t)rows * BK;
    dim3 grid2((unsigned)((total + 255) / 256)), block2(256);
    BMF_LAUNCH(masked_link_rows_wide_kernel, grid2, block2, 0, s, row_seg_ptr, rows, part0, num0, den0);
    BMF_LAUNCH(masked_link_rows_wide_kernel, grid2, block2, 0, s, row_seg_ptr, rows, part1, num1, den1);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}
