// Factor expansion, rebuild and overlap pruning of GreConD+ on bit sets (PyBMF/models/GreConDPlus.py:131-308), exact integer work; the
// one fp64 expression is the reference's, products and sums in its order (this file is built with -ffp-contract=off: never an FMA).
//
// A bit matrix is `lines` bit rows of ld words, zero padded: X / RS row-major (line = row of X, the set s = v) or transposed (line =
// column of X, s = u).  RS = X & ~PD is the residual the expansion holds fixed.
//   counts   a_l = |RS_l|, b_l = |X_l & (RS_l | s)|, c_l = |s & ~X_l|                                          (expand_counts_kernel)
//   steps    d_l = ((-w_fp) c_l + w_fn b_l) - ((-w_fp) 0 + w_fn a_l), 0.0 for a line inside its own set; r = the FIRST row of the highest
//            d, c = the first column; r_score > c_score and > 0: the row joins u, u_exp and every column counter takes the row's bit
//            (b += x & ~rs, c += ~x); c_score > r_score and > 0: the column likewise; otherwise stop          (expand_steps_kernel)
//   rebuild  PD_l = OR of S[f] over the factors f whose member set M[f] holds l, RS_l = X_l & ~PD_l, |RS_l| and their sum
//                                                                                                              (bits_rebuild_kernel)
//   subset   flag[p] = S[set[p]] is inside X[line[p]]                                                          (bits_subset_kernel)
//   overlap  cov[i][j] = the number of factors with U[f] holding i and V[f] holding j                          (overlap_counts_kernel)
//   prune    the rows of u_exp whose cells over v are all ones of X covered twice leave u and u_exp, their counts over v drop by one;
//            then the columns of v_exp likewise over the rows u held BEFORE the row pass           (overlap_rows_kernel, overlap_cols_kernel)
// Integer adds in a fixed order; the only atomics clear single bits of a word that several lines share.
#include "bits_common.h"

namespace {

constexpr int STEP_THREADS = 1024;

// One wave per line, 4 lines per block, 16-byte loads.
__global__ __launch_bounds__(256) void expand_counts_kernel(const uint4* __restrict__ X, const uint4* __restrict__ RS, int lines, int ld4,
                                                            const uint4* __restrict__ s, int32_t* __restrict__ a, int32_t* __restrict__ b,
                                                            int32_t* __restrict__ c) {
    const int lane = threadIdx.x & 63, l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= lines) return;
    const int64_t base = (int64_t)l * ld4;
    uint32_t ca = 0, cb = 0, cc = 0;
#pragma unroll 2
    for (int w = lane; w < ld4; w += 64) {
        const uint4 x = X[base + w], r = RS[base + w], sv = s[w];
        ca += popc4(r);
        cb += popc4(make_uint4(x.x & (r.x | sv.x), x.y & (r.y | sv.y), x.z & (r.z | sv.z), x.w & (r.w | sv.w)));
        cc += popc4(make_uint4(sv.x & ~x.x, sv.y & ~x.y, sv.z & ~x.z, sv.w & ~x.w));
    }
    ca = wave_sum(ca);
    cb = wave_sum(cb);
    cc = wave_sum(cc);
    if (lane == 0) {
        a[l] = (int32_t)ca;
        b[l] = (int32_t)cb;
        c[l] = (int32_t)cc;
    }
}

__device__ inline double expand_score(double w_fp, double w_fn, int a, int b, int c) {
    const double s_new = (-w_fp) * (double)c + w_fn * (double)b;
    const double s_old = (-w_fp) * 0.0 + w_fn * (double)a;
    return s_new - s_old;
}

// (score, index) of the higher score, of equals the lower index
__device__ inline void take_better(double& s, int& i, double s2, int i2) {
    if (s2 > s || (s2 == s && i2 < i)) {
        s = s2;
        i = i2;
    }
}

// The first index of the highest d over `lines` lines; set: the lines inside (d = 0.0).  The result is in every thread; two barriers.
__device__ inline void first_argmax(const int32_t* abc, int lines, const uint32_t* set, double w_fp, double w_fn, double* red_s, int* red_i,
                                    double& out_s, int& out_i) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double s = -INFINITY;
    int idx = 0x7fffffff;
    for (int l = t; l < lines; l += STEP_THREADS) {
        const bool inside = (set[l >> 5] >> (l & 31)) & 1u;
        const double d = inside ? 0.0 : expand_score(w_fp, w_fn, abc[l], abc[lines + l], abc[2 * (int64_t)lines + l]);
        if (d > s) {        // ascending l in a thread: strict > keeps the first
            s = d;
            idx = l;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) take_better(s, idx, __shfl_xor(s, o), __shfl_xor(idx, o));
    if (lane == 0) {
        red_s[wave] = s;
        red_i[wave] = idx;
    }
    __syncthreads();
    s = red_s[0];
    idx = red_i[0];
    for (int w = 1; w < STEP_THREADS / 64; ++w) take_better(s, idx, red_s[w], red_i[w]);
    __syncthreads();
    out_s = s;
    out_i = idx;
}

// One workgroup runs up to `budget` steps.  rec[0] = joins so far, rec[1] = 1 once stopped, rec[2] = steps evaluated (joins + the stop),
// rec[3] = 0; step e writes rec[4 + 4 e ..] = { axis (1: a row joined, 0: a column, -1: stop), index, bits of r_score, bits of c_score }.
// The counters and the four sets live in HBM between launches; nothing is written once rec[1] is set.
__global__ __launch_bounds__(STEP_THREADS) void expand_steps_kernel(const uint32_t* __restrict__ x, const uint32_t* __restrict__ rs,
                                                                    const uint32_t* __restrict__ x_t, const uint32_t* __restrict__ rs_t, int m,
                                                                    int n, int ldx, int ldw, double w_fp, double w_fn, int budget,
                                                                    int32_t* row_abc, int32_t* col_abc, uint32_t* u, uint32_t* v,
                                                                    uint32_t* u_exp, uint32_t* v_exp, int64_t* rec) {
    __shared__ double red_s[STEP_THREADS / 64];
    __shared__ int red_i[STEP_THREADS / 64];
    const int t = threadIdx.x;
    if (rec[1] != 0) return;        // (uniform)
    int64_t done = rec[0], seen = rec[2];
    const int64_t cap = (int64_t)m + n + 1;
    for (int step = 0; step < budget && seen < cap; ++step) {
        double r_score, c_score;
        int r_index, c_index;
        first_argmax(row_abc, m, u, w_fp, w_fn, red_s, red_i, r_score, r_index);
        first_argmax(col_abc, n, v, w_fp, w_fn, red_s, red_i, c_score, c_index);
        int axis = -1;
        if (r_score > c_score && r_score > 0.0) axis = 1;
        else if (c_score > r_score && c_score > 0.0) axis = 0;
        if (done >= (int64_t)m + n) axis = -1;     // every line has joined: nothing can score above 0
        const int index = axis == 1 ? r_index : c_index;
        if (t == 0) {
            int64_t* e = rec + 4 + 4 * seen;
            e[0] = axis;
            e[1] = axis == 1 ? r_index : (axis == 0 ? c_index : -1);
            e[2] = __double_as_longlong(r_score);
            e[3] = __double_as_longlong(c_score);
        }
        ++seen;
        if (axis < 0) {
            if (t == 0) {
                rec[1] = 1;
                rec[2] = seen;
            }
            return;
        }
        ++done;
        if (axis == 1) {     // row `index` joins u: the column counters take its cells
            if (t == 0) {
                u[index >> 5] |= 1u << (index & 31);
                u_exp[index >> 5] |= 1u << (index & 31);
            }
            const uint32_t* xr = x + (int64_t)index * ldx;
            const uint32_t* rr = rs + (int64_t)index * ldx;
            for (int j = t; j < n; j += STEP_THREADS) {
                const uint32_t xb = (xr[j >> 5] >> (j & 31)) & 1u, rb = (rr[j >> 5] >> (j & 31)) & 1u;
                col_abc[n + j] += (int32_t)(xb & ~rb & 1u);
                col_abc[2 * (int64_t)n + j] += (int32_t)(xb ^ 1u);
            }
        } else {             // column `index` joins v: the row counters take its cells
            if (t == 0) {
                v[index >> 5] |= 1u << (index & 31);
                v_exp[index >> 5] |= 1u << (index & 31);
            }
            const uint32_t* xc = x_t + (int64_t)index * ldw;
            const uint32_t* rc = rs_t + (int64_t)index * ldw;
            for (int i = t; i < m; i += STEP_THREADS) {
                const uint32_t xb = (xc[i >> 5] >> (i & 31)) & 1u, rb = (rc[i >> 5] >> (i & 31)) & 1u;
                row_abc[m + i] += (int32_t)(xb & ~rb & 1u);
                row_abc[2 * (int64_t)m + i] += (int32_t)(xb ^ 1u);
            }
        }
        if (t == 0) {
            rec[0] = done;
            rec[2] = seen;
        }
        __syncthreads();     // the counters and the sets are in memory before the next step reads them
    }
}

// One wave per line, 4 lines per block.  M[f * ldm + (l >> 5)] bit l & 31: factor f holds line l.
__global__ __launch_bounds__(256) void bits_rebuild_kernel(const uint32_t* __restrict__ X, int lines, int ld, const uint32_t* __restrict__ S,
                                                           const uint32_t* __restrict__ M, int ldm, int f, uint32_t* __restrict__ PD,
                                                           uint32_t* __restrict__ RS, int32_t* __restrict__ count) {
    const int lane = threadIdx.x & 63, l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= lines) return;
    const int64_t base = (int64_t)l * ld;
    uint32_t cnt = 0;
    for (int w0 = 0; w0 < ld; w0 += 64) {
        const int w = w0 + lane;
        uint32_t pd = 0;
        for (int k = 0; k < f; ++k)
            if (((M[(int64_t)k * ldm + (l >> 5)] >> (l & 31)) & 1u) && w < ld) pd |= S[(int64_t)k * ld + w];
        if (w < ld) {
            const uint32_t r = X[base + w] & ~pd;
            if (PD) PD[base + w] = pd;
            RS[base + w] = r;
            cnt += __popc(r);
        }
    }
    cnt = wave_sum(cnt);
    if (lane == 0 && count) count[l] = (int32_t)cnt;
}

// One wave per pair, 4 per block.  A pair outside the matrices is flagged 0.
__global__ __launch_bounds__(256) void bits_subset_kernel(const uint32_t* __restrict__ X, int lines, int ld, const uint32_t* __restrict__ S, int f,
                                                          const int32_t* __restrict__ line, const int32_t* __restrict__ set, int count,
                                                          int32_t* __restrict__ flag) {
    const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= count) return;
    const int l = line[p], k = set[p];
    bool ok = l >= 0 && l < lines && k >= 0 && k < f;
    if (ok) {
        uint32_t out = 0;
        for (int w = lane; w < ld; w += 64) out |= S[(int64_t)k * ld + w] & ~X[(int64_t)l * ld + w];
        ok = __ballot(out != 0) == 0ull;
    }
    if (lane == 0) flag[p] = ok ? 1 : 0;
}

// One thread per cell.
__global__ __launch_bounds__(256) void overlap_counts_kernel(const uint32_t* __restrict__ Ub, int ldu, const uint32_t* __restrict__ Vb, int ldv,
                                                             int f, int m, int n, int32_t* __restrict__ cov, int64_t ldc) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= n || i >= m) return;
    int32_t c = 0;
    for (int k = 0; k < f; ++k)
        c += (int32_t)((Ub[(int64_t)k * ldu + (i >> 5)] >> (i & 31)) & (Vb[(int64_t)k * ldv + (j >> 5)] >> (j & 31)) & 1u);
    cov[(int64_t)i * ldc + j] = c;
}

// One wave per row of u_exp, 4 rows per block; v is only read here.  A row touches its own line of cov alone.
__global__ __launch_bounds__(256) void overlap_rows_kernel(const uint32_t* __restrict__ x, int ldx, int m, int n, int32_t* cov, int64_t ldc,
                                                           uint32_t* u, uint32_t* u_exp, const uint32_t* __restrict__ v) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m || !((u_exp[i >> 5] >> (i & 31)) & 1u)) return;
    bool ok = true;
    for (int j = lane; j < n; j += 64)
        if ((v[j >> 5] >> (j & 31)) & 1u) ok = ok && ((x[(int64_t)i * ldx + (j >> 5)] >> (j & 31)) & 1u) && cov[(int64_t)i * ldc + j] >= 2;
    if (__ballot(!ok) != 0ull) return;
    for (int j = lane; j < n; j += 64)
        if ((v[j >> 5] >> (j & 31)) & 1u) cov[(int64_t)i * ldc + j] -= 1;
    if (lane == 0) {
        atomicAnd(&u[i >> 5], ~(1u << (i & 31)));
        atomicAnd(&u_exp[i >> 5], ~(1u << (i & 31)));
    }
}

// One wave per column of v_exp, 4 per block; u_old: the rows u held before the row pass.  A column touches its own cells of cov alone.
__global__ __launch_bounds__(256) void overlap_cols_kernel(const uint32_t* __restrict__ x, int ldx, int m, int n, int32_t* cov, int64_t ldc,
                                                           const uint32_t* __restrict__ u_old, uint32_t* v, uint32_t* v_exp) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n || !((v_exp[j >> 5] >> (j & 31)) & 1u)) return;
    bool ok = true;
    for (int i = lane; i < m; i += 64)
        if ((u_old[i >> 5] >> (i & 31)) & 1u) ok = ok && ((x[(int64_t)i * ldx + (j >> 5)] >> (j & 31)) & 1u) && cov[(int64_t)i * ldc + j] >= 2;
    if (__ballot(!ok) != 0ull) return;
    for (int i = lane; i < m; i += 64)
        if ((u_old[i >> 5] >> (i & 31)) & 1u) cov[(int64_t)i * ldc + j] -= 1;
    if (lane == 0) {
        atomicAnd(&v[j >> 5], ~(1u << (j & 31)));
        atomicAnd(&v_exp[j >> 5], ~(1u << (j & 31)));
    }
}

}  // namespace

extern "C" int bmf_expand_counts(const uint32_t* X, const uint32_t* RS, int32_t lines, int64_t ld, const uint32_t* s, int32_t* abc,
                                 void* stream) {
    BMF_REQUIRE(X && RS && s && abc, "bmf_expand_counts: null pointer");
    BMF_REQUIRE(lines >= 1, "bmf_expand_counts: need lines >= 1");
    BMF_REQUIRE(ld_ok(ld), "bmf_expand_counts: ld must be a multiple of 4 words, at most 2^26");
    BMF_REQUIRE(bmf_aligned16(X) && bmf_aligned16(RS) && bmf_aligned16(s), "bmf_expand_counts: X, RS and s must be 16-byte aligned");
    BMF_REQUIRE(aligned4(abc), "bmf_expand_counts: abc must be 4-byte aligned");
    BMF_LAUNCH(expand_counts_kernel, dim3((unsigned)((lines + 3) / 4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(X),
               reinterpret_cast<const uint4*>(RS), lines, (int)(ld / 4), reinterpret_cast<const uint4*>(s), abc, abc + lines,
               abc + 2 * (int64_t)lines);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int64_t bmf_expand_rec_words(int32_t m, int32_t n) {
    if (m < 1 || n < 1) return BMF_ERR_BAD_ARG;
    return 4 + 4 * ((int64_t)m + n + 1);
}

extern "C" int bmf_expand_steps(const uint32_t* x, const uint32_t* rs, const uint32_t* x_t, const uint32_t* rs_t, int32_t m, int32_t n,
                                int64_t ldx, int64_t ldw, double w_fp, double w_fn, int32_t steps, int32_t* row_abc, int32_t* col_abc,
                                uint32_t* u, uint32_t* v, uint32_t* u_exp, uint32_t* v_exp, int64_t* rec, void* stream) {
    BMF_REQUIRE(x && rs && x_t && rs_t && row_abc && col_abc && u && v && u_exp && v_exp && rec, "bmf_expand_steps: null pointer");
    BMF_REQUIRE(m >= 1 && n >= 1 && steps >= 1, "bmf_expand_steps: need m >= 1, n >= 1 and steps >= 1");
    BMF_REQUIRE(ldx >= 1 && ldx <= (1 << 26) && (int64_t)n <= 32 * ldx, "bmf_expand_steps: the rows need 1 <= ldx <= 2^26 and n <= 32 * ldx");
    BMF_REQUIRE(ldw >= 1 && ldw <= (1 << 26) && (int64_t)m <= 32 * ldw, "bmf_expand_steps: the columns need 1 <= ldw <= 2^26 and m <= 32 * ldw");
    BMF_REQUIRE(w_fp == w_fp && w_fn == w_fn && w_fp - w_fp == 0.0 && w_fn - w_fn == 0.0, "bmf_expand_steps: the weights must be finite");
    BMF_REQUIRE(aligned4(row_abc) && aligned4(col_abc) && aligned8(rec), "bmf_expand_steps: the counters must be 4-byte, rec 8-byte aligned");
    BMF_LAUNCH(expand_steps_kernel, dim3(1), dim3(STEP_THREADS), 0, (hipStream_t)stream, x, rs, x_t, rs_t, m, n, (int)ldx, (int)ldw, w_fp, w_fn,
               steps, row_abc, col_abc, u, v, u_exp, v_exp, rec);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_bits_rebuild(const uint32_t* X, int32_t lines, int64_t ld, const uint32_t* S, const uint32_t* M, int64_t ldm, int32_t f,
                                uint32_t* PD, uint32_t* RS, int32_t* count, int64_t* sum, void* stream) {
    BMF_REQUIRE(X && RS, "bmf_bits_rebuild: null pointer");
    BMF_REQUIRE(f >= 0 && (f == 0 || (S && M)), "bmf_bits_rebuild: f >= 0 factors, with their sets S and member sets M when f > 0");
    BMF_REQUIRE(lines >= 1 && ld >= 1 && ld <= (1 << 26), "bmf_bits_rebuild: need lines >= 1 and 1 <= ld <= 2^26");
    BMF_REQUIRE(f == 0 || (ldm >= 1 && (int64_t)lines <= 32 * ldm), "bmf_bits_rebuild: the member sets need lines <= 32 * ldm");
    BMF_REQUIRE((sum == nullptr) || count, "bmf_bits_rebuild: the sum is taken over count");
    BMF_REQUIRE(aligned4(count) && aligned8(sum), "bmf_bits_rebuild: count must be 4-byte, sum 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    BMF_LAUNCH(bits_rebuild_kernel, dim3((unsigned)((lines + 3) / 4)), dim3(256), 0, st, X, lines, (int)ld, S, M, (int)ldm, f, PD, RS, count);
    if (sum) bits_sum_launch(count, lines, sum, nullptr, st);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_bits_subset(const uint32_t* X, int32_t lines, int64_t ld, const uint32_t* S, int32_t f, const int32_t* line,
                               const int32_t* set, int32_t count, int32_t* flag, void* stream) {
    BMF_REQUIRE(X && S && line && set && flag, "bmf_bits_subset: null pointer");
    BMF_REQUIRE(lines >= 1 && f >= 1 && count >= 1, "bmf_bits_subset: need lines >= 1, f >= 1 and count >= 1");
    BMF_REQUIRE(ld >= 1 && ld <= (1 << 26), "bmf_bits_subset: need 1 <= ld <= 2^26");
    BMF_REQUIRE(aligned4(line) && aligned4(set) && aligned4(flag), "bmf_bits_subset: line, set and flag must be 4-byte aligned");
    BMF_LAUNCH(bits_subset_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, (hipStream_t)stream, X, lines, (int)ld, S, f, line, set, count,
               flag);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_overlap_counts(const uint32_t* Ub, int64_t ldu, const uint32_t* Vb, int64_t ldv, int32_t f, int32_t m, int32_t n,
                                  int32_t* cov, int64_t ldc, void* stream) {
    BMF_REQUIRE(Ub && Vb && cov, "bmf_overlap_counts: null pointer");
    BMF_REQUIRE(f >= 1 && m >= 1 && n >= 1 && m <= 65535, "bmf_overlap_counts: need f >= 1, 1 <= m <= 65535 and n >= 1");
    BMF_REQUIRE(ldu >= 1 && ldu <= (1 << 26) && (int64_t)m <= 32 * ldu, "bmf_overlap_counts: U needs m <= 32 * ldu");
    BMF_REQUIRE(ldv >= 1 && ldv <= (1 << 26) && (int64_t)n <= 32 * ldv, "bmf_overlap_counts: V needs n <= 32 * ldv");
    BMF_REQUIRE(ldc >= n && aligned4(cov), "bmf_overlap_counts: cov needs ldc >= n and 4-byte alignment");
    BMF_LAUNCH(overlap_counts_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)m), dim3(256), 0, (hipStream_t)stream, Ub, (int)ldu, Vb, (int)ldv,
               f, m, n, cov, ldc);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_overlap_prune(const uint32_t* x, int64_t ldx, int32_t m, int32_t n, int32_t* cov, int64_t ldc, uint32_t* u,
                                 uint32_t* u_exp, uint32_t* v, uint32_t* v_exp, uint32_t* u_old, int64_t ldw, void* stream) {
    BMF_REQUIRE(x && cov && u && u_exp && v && v_exp && u_old, "bmf_overlap_prune: null pointer");
    BMF_REQUIRE(m >= 1 && n >= 1, "bmf_overlap_prune: need m >= 1 and n >= 1");
    BMF_REQUIRE(ldx >= 1 && ldx <= (1 << 26) && (int64_t)n <= 32 * ldx, "bmf_overlap_prune: the rows need n <= 32 * ldx");
    BMF_REQUIRE(ldw >= 1 && ldw <= (1 << 26) && (int64_t)m <= 32 * ldw, "bmf_overlap_prune: the row sets need m <= 32 * ldw");
    BMF_REQUIRE(ldc >= n && aligned4(cov), "bmf_overlap_prune: cov needs ldc >= n and 4-byte alignment");
    BMF_REQUIRE(u_old != u, "bmf_overlap_prune: u_old is a copy of u, not u");
    hipStream_t st = (hipStream_t)stream;
    BMF_HIP_CHECK(hipMemcpyAsync(u_old, u, (size_t)ldw * 4, hipMemcpyDeviceToDevice, st));
    BMF_LAUNCH(overlap_rows_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, x, (int)ldx, m, n, cov, ldc, u, u_exp, v);
    BMF_LAUNCH(overlap_cols_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, x, (int)ldx, m, n, cov, ldc, u_old, v, v_exp);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}
