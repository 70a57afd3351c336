// The proximal (PALM / iPALM) step of ELBMF and PRIMP at a rank 64 < k <= 128 (PyBMF/models/ELBMF.py:177-210, PRIMP.py:51-88; the
// reference has no rank limit).  A factor is two blocks of 64 columns, F = [F_0 | F_1] (pybmf_amd/wide.py); everything per column runs
// per block through the kernels of the k <= 64 path.  What couples the blocks is here:
//
//   bmf_sym_norms_wide      spectral and Frobenius norm of the 128 x 128 Gram (the Lipschitz constants of the step sizes)
//   bmf_palm_epilogue_wide  one step of both blocks of a factor: Fe (G^T G) needs the cross blocks of the Gram, so the product runs
//                           over all 128 columns before either block is written
//
// The norm kernel's plan.  The 64-column kernel (palm.hip) keeps three fp64 copies of the matrix in LDS: iterate, squared iterate, and
// the input for the Rayleigh quotient.  At 128 x 128 one copy is 128 KiB of the 160 KiB a compute unit has, so this kernel keeps ONE:
// every thread holds its 8 x 8 tile of the squared iterate in registers (64 doubles), and once the whole block has finished reading
// the iterate (a barrier) the tiles are written over it in place.  The quotient v^T G v / v^T v needs no copy of the input either: a
// quadratic form does not see the antisymmetric part of G, so it is one coalesced pass over G in global memory.  One workgroup, no
// grid barrier, no atomics: every sum runs in a fixed order.
#include "common.h"

namespace {

constexpr int WN = 128;              // side of the wide Gram
constexpr int WTS = 8;               // tile side per thread: 16 x 16 threads
constexpr int NORM_SQUARINGS = 32;   // as bmf_sym_norms: the dominant direction amplified 2^32-fold

__global__ __launch_bounds__(256) void sym_norms_wide_kernel(const double* __restrict__ G, double* __restrict__ out) {
    __shared__ __attribute__((aligned(32))) double A[WN][WN];
    __shared__ double red[2][4];
    __shared__ int jmax_s;
    const int t = threadIdx.x, ti = (t >> 4) * WTS, tj = (t & 15) * WTS;
    const int wave = t >> 6;

    auto block_sum2 = [&](double& v0, double& v1) {
        v0 = wave_sum(v0);
        v1 = wave_sum(v1);
        __syncthreads();   // (the previous call's readers are done -- and so is every reader of A before this call)
        if ((t & 63) == 0) { red[0][wave] = v0; red[1][wave] = v1; }
        __syncthreads();
        v0 = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        v1 = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    };

    double fro = 0.0, tr = 0.0;
    for (int e = t; e < WN * WN; e += 256) {
        const double g = G[e];
        fro += g * g;
        if (e / WN == e % WN) tr += g;
    }
    block_sum2(fro, tr);
    if (!(tr > 0.0)) {  // the zero matrix (an all-zero factor)
        if (t == 0) {
            out[0] = 0.0;
            out[1] = sqrt(fro);
        }
        return;
    }
    // symmetrised and brought to trace 1 on the way in (the row trick below needs A[i][q] = A[q][i] bit for bit)
#pragma unroll
    for (int a = 0; a < WTS; ++a)
#pragma unroll
        for (int b = 0; b < WTS; ++b) A[ti + a][tj + b] = 0.5 * (G[(ti + a) * WN + tj + b] + G[(tj + b) * WN + ti + a]) / tr;
    __syncthreads();

    for (int it = 0; it < NORM_SQUARINGS; ++it) {
        double c[WTS][WTS];
#pragma unroll
        for (int a = 0; a < WTS; ++a)
#pragma unroll
            for (int b = 0; b < WTS; ++b) c[a][b] = 0.0;
        // both operands of a tile from ROW q (the iterate is symmetric): two aligned 64-byte reads per reduction index; the 16 lanes
        // of a wave that share `ti` read one address (broadcast), the 16 values of `tj` cover the row once (no bank conflict)
#pragma unroll 2
        for (int q = 0; q < WN; ++q) {
            double x[WTS], y[WTS];
#pragma unroll
            for (int a = 0; a < WTS; ++a) x[a] = A[q][ti + a];
#pragma unroll
            for (int b = 0; b < WTS; ++b) y[b] = A[q][tj + b];
#pragma unroll
            for (int a = 0; a < WTS; ++a)
#pragma unroll
                for (int b = 0; b < WTS; ++b) c[a][b] = fma(x[a], y[b], c[a][b]);
        }
        double d = 0.0, unused = 0.0;
        if (ti == tj) {
#pragma unroll
            for (int a = 0; a < WTS; ++a) d += c[a][a];
        }
        block_sum2(d, unused);   // (its first barrier: every thread has its whole tile, nobody reads A any more)
        const double trace = d;  // > 0: the square of a non-zero symmetric matrix has a positive trace
        const double inv = 1.0 / trace;
        // c[a][b] and the mirrored tile's c[b][a] are sums of the same products in the same order: A stays symmetric bit for bit
#pragma unroll
        for (int a = 0; a < WTS; ++a)
#pragma unroll
            for (int b = 0; b < WTS; ++b) A[ti + a][tj + b] = c[a][b] * inv;
        __syncthreads();
        // the iterate that was squared had trace 1, so tr(A^2) = 1 - 2 eps + O(eps^2), eps = the weight of the other directions; the one
        // just written has eps^2 and the quotient below is off by O(eps^4) (palm.hip).  Block-uniform.
        if (trace >= 1.0 - 1.0e-5) break;
    }
    // v = the column of the amplified matrix with the largest diagonal entry (first wave: lane j looks at entries j and j + 64, the
    // lower index wins a tie), then the Rayleigh quotient of the INPUT: v^T G v over all 128 x 128 entries, coalesced
    if (t < 64) {
        double dv = A[t][t];
        int dj = t;
        if (A[t + 64][t + 64] > dv) { dv = A[t + 64][t + 64]; dj = t + 64; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(dv, o, 64);
            const int oj = __shfl_xor(dj, o, 64);
            if (ov > dv || (ov == dv && oj < dj)) { dv = ov; dj = oj; }
        }
        if (t == 0) jmax_s = dj;
    }
    __syncthreads();
    const int jm = jmax_s;
    double num = 0.0, den = 0.0;
    {
        const int col = t & (WN - 1);           // e % WN is the same for every e = t + 256 i
        const double vc = A[jm][col];
#pragma unroll 8
        for (int i = 0; i < WN * WN / 256; ++i) {
            const int e = t + 256 * i;
            num = fma(G[e] * A[jm][e / WN], vc, num);
        }
        if (t < WN) den = vc * vc;
    }
    block_sum2(num, den);
    if (t == 0) {
        out[0] = num / den;
        out[1] = sqrt(fro);
    }
}

__device__ __forceinline__ double sgn(double x) { return (double)((x > 0.0) - (x < 0.0)); }
// proxelbmf (PRIMP.py:55-56) = the inner expression of prox (ELBMF.py:203-208); the expression of palm.hip
__device__ __forceinline__ double prox_core(double x, double kai, double lam) {
    const double p = x <= 0.5 ? x - kai * sgn(x) : x - kai * sgn(x - 1.0) + lam;
    return p / (1.0 + lam);
}

// One block = 128 rows = 4 waves x 32 rows, the tiling of palm_epilogue_kernel (palm.hip).  Fe G for BOTH output blocks first -- a
// wave multiplies its own 32 rows of Fe = [Fe_0 | Fe_1] (fp32 from the fp64 masters) by the four 64 x 64 blocks of G on the exact-fp32
// MFMA (v_mfma_f32_32x32x2_f32: 256 per wave, 64 accumulator registers) -- and only then the element-wise step of block 0 and of
// block 1 in fp64, in the C/D layout of the product: the step writes the masters the product reads.
__global__ __launch_bounds__(256) void palm_epilogue_wide_kernel(bmf_palm_wide_args a) {
    constexpr int BK = 64, KH = 32, NT = 2;
    __shared__ double red[2][4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * 128 + wave * 32;
    const double beta = a.beta;

    const double L = fmax(a.norms[a.norm_kind == BMF_NORM_SPECTRAL ? 0 : 1], 1e-4);
    const double eta = beta == 0.0 ? 1.0 / (1.1 * L) : 2.0 * (1.0 - beta) / (1.0 + 2.0 * beta) / L;
    const double kai = a.l1 * eta, lam = a.l2 * eta;

    // ---- Fe G: A = (float)Fe_ab[row c][KH h + s], B = G[ab][b][KH h + s][32 nt + c] ----
    f32x16 fg[2][NT];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) fg[b][nt][i] = 0.f;
#pragma unroll
    for (int ab = 0; ab < 2; ++ab) {
        const double* fp = a.F64[ab] + (row0 + c) * BK + KH * h;
        const double* pp = a.Fprev64[ab] + (row0 + c) * BK + KH * h;
#pragma unroll
        for (int s0 = 0; s0 < KH; s0 += 8) {
            float av[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const double f = fp[s0 + s];
                av[s] = (float)(beta == 0.0 ? f : f + beta * (f - pp[s0 + s]));
            }
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const float* g = a.G[ab][b] + (KH * h + s0) * BK + c;
                float gv[NT][8];
#pragma unroll
                for (int s = 0; s < 8; ++s)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) gv[nt][s] = g[s * BK + 32 * nt];
#pragma unroll
                for (int s = 0; s < 8; ++s)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) fg[b][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], gv[nt][s], fg[b][nt], 0, 0, 0);
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);   // (no store of the step below may move above a load of the product)

#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int kb = b == 0 ? BK : a.k - BK;   // real columns of this block
        double* F64 = a.F64[b];
        double* P64 = a.Fprev64[b];
        float* F = a.F[b];
        const float* numb = a.num[b];
        double gap_acc = 0.0;
        unsigned colword[NT] = {0u, 0u};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int rl = (i & 3) + 8 * (i >> 2) + 4 * h;
            const int64_t r = row0 + rl;
            const bool row_ok = r < a.rows;
            unsigned long long ball[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = 32 * nt + c;
                const bool ok = row_ok && col < kb;
                const int64_t idx = r * BK + col;
                const double f = F64[idx];
                const double p = P64[idx];
                float num = 0.f;
                for (int sp = 0; sp < a.splits; ++sp) num += numb[(int64_t)sp * a.slab_stride + idx];
                const double fe = beta == 0.0 ? f : f + beta * (f - p);
                const double grad = (double)fg[b][nt][i] - (double)num;
                double x = fe - eta * grad;
                double fn;
                if (a.variant == BMF_PALM_ELBMF) {
                    fn = prox_core(x, kai, lam);
                    if (fn < 0.0) fn = 0.0;
                } else {  // PRIMP: proxelbmfnn then _proxelbmfnn
                    x = fmax(prox_core(x, kai, lam), 0.0);
                    fn = fmin(prox_core(x, kai, lam), 1.0);
                }
                if (!ok) fn = 0.0;
                F64[idx] = fn;
                if (a.advance_prev) P64[idx] = ok ? f : 0.0;
                F[idx] = (float)fn;
                if (ok) {
                    const double dist = fn < 0.5 ? fabs(fn) : fabs(fn - 1.0);
                    gap_acc += a.gap_l1 * dist + a.gap_l2 * dist * dist;
                }
                const bool bit = ok && (fn > (double)a.thr);
                ball[nt] = __ballot(bit);
                colword[nt] |= (bit ? 1u : 0u) << rl;
            }
            if (lane == 0) {
                const unsigned long long lo = (unsigned)ball[0] | ((unsigned long long)(unsigned)ball[1] << 32);
                const unsigned long long hi = (unsigned)(ball[0] >> 32) | ((unsigned long long)(unsigned)(ball[1] >> 32) << 32);
                const int64_t ra = row0 + (i & 3) + 8 * (i >> 2);
                a.rowbits[b][ra] = lo;
                a.rowbits[b][ra + 4] = hi;
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const unsigned w = colword[nt] | __shfl_xor(colword[nt], 32, 64);
            if (h == 0) a.colbits[b][(int64_t)(32 * nt + c) * a.ldcb + (row0 >> 5)] = w;
        }
        const double gs = wave_sum(gap_acc);
        if (lane == 0) red[b][wave] = gs;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.partials[0][blockIdx.x] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        a.partials[1][blockIdx.x] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

}  // namespace

extern "C" int bmf_sym_norms_wide(const double* G64, double* out, void* stream) {
    BMF_REQUIRE(G64 && out, "bmf_sym_norms_wide: null pointer");
    BMF_LAUNCH(sym_norms_wide_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, G64, out);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_palm_epilogue_wide(const bmf_palm_wide_args* a, void* stream) {
    BMF_REQUIRE(a, "bmf_palm_epilogue_wide: null args");
    BMF_REQUIRE(a->struct_bytes == (int32_t)sizeof(bmf_palm_wide_args), "bmf_palm_epilogue_wide: struct_bytes=%d, library expects %d", a->struct_bytes,
                (int)sizeof(bmf_palm_wide_args));
    for (int b = 0; b < 2; ++b)
        BMF_REQUIRE(a->F64[b] && a->Fprev64[b] && a->F[b] && a->num[b] && a->G[b][0] && a->G[b][1] && a->rowbits[b] && a->colbits[b] && a->partials[b],
                    "bmf_palm_epilogue_wide: null pointer");
    BMF_REQUIRE(a->norms, "bmf_palm_epilogue_wide: null pointer");
    BMF_REQUIRE(a->rows_pad > 0 && a->rows_pad % 128 == 0, "bmf_palm_epilogue_wide: rows_pad must be a multiple of 128");
    BMF_REQUIRE(a->rows >= 1 && a->rows <= a->rows_pad, "bmf_palm_epilogue_wide: rows out of range");
    BMF_REQUIRE(a->k > 64 && a->k <= 128, "bmf_palm_epilogue_wide: need 64 < k <= 128 (bmf_palm_epilogue takes k <= 64)");
    BMF_REQUIRE(a->splits >= 1 && a->slab_stride >= a->rows_pad * 64, "bmf_palm_epilogue_wide: bad slab description");
    BMF_REQUIRE(a->variant == BMF_PALM_ELBMF || a->variant == BMF_PALM_PRIMP, "bmf_palm_epilogue_wide: variant must be BMF_PALM_ELBMF or _PRIMP");
    BMF_REQUIRE(a->norm_kind == BMF_NORM_SPECTRAL || a->norm_kind == BMF_NORM_FROBENIUS, "bmf_palm_epilogue_wide: bad norm_kind");
    BMF_REQUIRE(a->beta >= 0.0 && a->beta < 1.0, "bmf_palm_epilogue_wide: beta must be in [0, 1)");
    BMF_REQUIRE(a->ldcb >= a->rows_pad / 32, "bmf_palm_epilogue_wide: ldcb too small");
    BMF_LAUNCH(palm_epilogue_wide_kernel, dim3((unsigned)(a->rows_pad / 128)), dim3(256), 0, (hipStream_t)stream, *a);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}
